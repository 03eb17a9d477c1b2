"""CPU: the backward of the grouped Downsample conv of RecNeXt-T / S / B (rcx_grouped_conv2d_bwd, ops.grouped_conv2d_backward, ops.GroupedConv2dFn,
ops.unpack_grouped_weight_grad): the declarations, the support and workspace queries, the argument errors that come before any HIP call, and the
refusal of CPU tensors."""
import ctypes
import os

import pytest
import torch

from recnext_amd import _lib, ops
from tests.test_ls_down_cpu import REGISTERED
from tests.util import GOLDEN

ENTRIES = ("rcx_grouped_conv2d_bwd_supported", "rcx_grouped_conv2d_bwd_workspace_bytes", "rcx_grouped_conv2d_bwd")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


def test_header_library_and_binding_have_the_three_entries(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "recnext_amd.h")) as f:
        header = f.read()
    for s in ENTRIES:
        assert hasattr(raw, s) and s in _lib.SIGNATURES and s + "(" in header, s
    assert lib.rcx_abi_version() == _lib.ABI_VERSION == 7                      # additions only
    doc = header[header.index("Backward of rcx_grouped_conv2d_fwd"):header.index("int rcx_grouped_conv2d_bwd_supported(")]
    assert "lsnet/model/recattn.py:254-263" in doc and "engine.py" in doc
    for f in ("grouped_conv2d_backward", "grouped_conv2d_backward_supported", "unpack_grouped_weight_grad", "GroupedConv2dFn"):
        assert getattr(ops, f).__module__ == "recnext_amd.lsdown", f
    makefile = open(os.path.join(os.path.dirname(GOLDEN), "..", "recnext_amd", "csrc", "Makefile")).read()
    tus = [l for l in makefile.splitlines() if l.startswith("SCRATCH_TUS")][0]
    assert "rcx_lsdownbwd" in tus.split()


def test_supported_agrees_with_the_forward_query(lib):
    fwd, bwd = lib.rcx_grouped_conv2d_supported, lib.rcx_grouped_conv2d_bwd_supported
    cases = [(n, side, side, cin, cout, g, 5, 2, dt) for cin, cout, g, side in REGISTERED for dt in (0, 1, 2) for n in (1, 2, 128, 256)]
    cases += [(1, 37, 50, cin, cout, g, 5, 2, 1) for cin, cout, g, _ in REGISTERED] + [(1, 1, 1, 8, 12, 4, 5, 2, 0)]
    cases += [(2, 9, 13, 70 * ci, 70 * co, 70, 5, 2, dt) for ci in (1, 2, 3, 4) for co in (1, 2, 3, 4) for dt in (0, 1, 2)]
    for c in cases:
        assert fwd(*c) == 1 and bwd(*c) == 1, c
    refused = [(2, 14, 14, 256, 384, 128, 3, 2, 1), (2, 14, 14, 256, 384, 128, 5, 1, 1), (2, 14, 14, 80, 32, 16, 5, 2, 1), (2, 14, 14, 32, 80, 16, 5, 2, 1),
               (2, 14, 14, 250, 384, 128, 5, 2, 1), (2, 14, 14, 256, 380, 128, 5, 2, 1), (2, 14, 14, 256, 384, 128, 5, 2, 3), (0, 14, 14, 256, 384, 128, 5, 2, 1)]
    for c in refused:                                                          # k, stride, ci, co, divisibility, dtype, an empty batch
        assert fwd(*c) == 0 and bwd(*c) == 0, c
        assert lib.rcx_grouped_conv2d_bwd_workspace_bytes(*c) == 0, c
    assert ops.grouped_conv2d_backward_supported(2, 14, 14, 256, 384, 128, 5, 2, torch.bfloat16)
    assert not ops.grouped_conv2d_backward_supported(2, 14, 14, 256, 384, 128, 5, 2, torch.float64)


def test_workspace_query_is_positive_deterministic_and_a_function_of_its_arguments(lib):
    q = lib.rcx_grouped_conv2d_bwd_workspace_bytes
    for cin, cout, g, side in REGISTERED:
        ci = cin // g
        row = 4 * (25 * ci + 1) * cout                                         # one partial: (25 ci + 1, Cout) float32
        for dt in (0, 1, 2):
            for n in (1, 2, 128):
                a = q(n, side, side, cin, cout, g, 5, 2, dt)
                assert a > 0 and a % row == 0 and a == q(n, side, side, cin, cout, g, 5, 2, dt), (cin, cout, side, dt, n)
                assert 1 <= a // row <= 512                                     # P partials
        assert q(1, side, side, cin, cout, g, 5, 2, 1) <= q(128, side, side, cin, cout, g, 5, 2, 1)
    assert q(128, 28, 28, 128, 256, 128, 5, 2, 1) // (4 * 26 * 256) >= 128       # batch 128: some hundreds of workgroups over the channel blocks


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(7)]                  # distinct, aligned, never dereferenced: the checks come first
    x, gy, wp, gx, gw, gb, ws = p
    bwd = lib.rcx_grouped_conv2d_bwd
    shape = (2, 14, 14, 256, 384, 128, 5, 2, 1)
    need = lib.rcx_grouped_conv2d_bwd_workspace_bytes(*shape)
    ok_tail = (ws, need) + shape + (None,)
    assert bwd(None, gy, wp, gx, gw, gb, *ok_tail) == _lib.ERR_BAD_ARG
    assert b"null" in lib.rcx_last_error()
    assert bwd(x, None, wp, gx, gw, gb, *ok_tail) == _lib.ERR_BAD_ARG
    assert bwd(x, gy, None, gx, gw, gb, *ok_tail) == _lib.ERR_BAD_ARG
    assert bwd(x, gy, wp, None, None, None, *ok_tail) == _lib.ERR_BAD_ARG    # nothing asked for
    assert b"every output" in lib.rcx_last_error()
    for out in ((x, gw, gb), (gx, gy, gb), (gx, gw, wp), (gx, gx, gb), (gx, gw, gw), (ws, gw, gb), (gx, ws, gb), (gx, gw, ws)):
        assert bwd(x, gy, wp, *out, *ok_tail) == _lib.ERR_BAD_ARG, out       # an output aliases an input, another output or the workspace
        assert b"alias" in lib.rcx_last_error()
    assert bwd(x, gy, wp, gx, gw, gb, x, need, *shape, None) == _lib.ERR_BAD_ARG             # the workspace aliases an input
    assert bwd(x, gy, wp, gx, gw, gb, ws, need, 2, 14, 14, 256, 384, 128, 5, 2, 9, None) == _lib.ERR_BAD_ARG      # dtype
    assert b"dtype" in lib.rcx_last_error()
    assert bwd(x, gy, wp, gx, gw, gb, ws, need, 2, 0, 14, 256, 384, 128, 5, 2, 1, None) == _lib.ERR_BAD_ARG
    assert bwd(x, gy, wp, gx, gw, gb, ws, need, 2, 14, 14, 256, 384, 0, 5, 2, 1, None) == _lib.ERR_BAD_ARG
    for i in range(7):                                                        # half an element / half a float
        q = list(p)
        q[i] = ctypes.c_void_p(p[i].value + (1 if i in (0, 1, 3) else 2))
        assert bwd(*q[:6], q[6], need, *shape, None) == _lib.ERR_BAD_ARG, i
        assert b"aligned" in lib.rcx_last_error()
    # a workspace smaller than the query, or none, where a weight or bias gradient is asked for
    assert bwd(x, gy, wp, gx, gw, gb, ws, need - 1, *shape, None) == _lib.ERR_WORKSPACE
    assert b"workspace" in lib.rcx_last_error()
    assert bwd(x, gy, wp, gx, gw, None, None, 0, *shape, None) == _lib.ERR_WORKSPACE
    assert bwd(x, gy, wp, None, None, gb, ws, 0, *shape, None) == _lib.ERR_WORKSPACE
    # geometry without a kernel
    assert bwd(x, gy, wp, gx, gw, gb, ws, need, 2, 14, 14, 256, 384, 128, 3, 2, 1, None) == _lib.ERR_UNSUPPORTED      # k = 3
    assert bwd(x, gy, wp, gx, gw, gb, ws, need, 2, 14, 14, 256, 384, 128, 5, 1, 1, None) == _lib.ERR_UNSUPPORTED      # stride 1
    assert bwd(x, gy, wp, gx, gw, gb, ws, need, 2, 14, 14, 80, 32, 16, 5, 2, 1, None) == _lib.ERR_UNSUPPORTED         # ci = 5
    assert bwd(x, gy, wp, gx, gw, gb, ws, need, 2, 14, 14, 250, 384, 128, 5, 2, 1, None) == _lib.ERR_UNSUPPORTED      # Cin % groups
    assert b"groups" in lib.rcx_last_error()


def test_unpack_is_the_inverse_of_pack():
    w = torch.randn(20, 3, 5, 5, generator=torch.Generator().manual_seed(0))
    back = ops.unpack_grouped_weight_grad(ops.pack_grouped_weight(w))
    assert tuple(back.shape) == (20, 3, 5, 5) and back.is_contiguous() and torch.equal(back, w)
    with pytest.raises(ValueError):
        ops.unpack_grouped_weight_grad(w[0])


def test_backward_and_the_function_refuse_a_cpu_tensor():
    w = torch.randn(64, 3, 5, 5)
    wp = ops.pack_grouped_weight(w)
    x, gy = torch.randn(1, 48, 7, 7), torch.randn(1, 64, 4, 4)
    with pytest.raises(_lib.RcxError):
        ops.grouped_conv2d_backward(x, gy, wp, 16)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_backward(x[0], gy, wp, 16)
    with pytest.raises(ValueError):
        ops.grouped_conv2d_backward(x.double(), gy.double(), wp, 16)
    with pytest.raises(_lib.RcxError):
        ops.GroupedConv2dFn.apply(x.requires_grad_(True), w.requires_grad_(True), None, 16)
