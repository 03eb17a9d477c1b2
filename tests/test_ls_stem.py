"""CPU: the T / S / B stem's HIP path (rcx_stem3_*, ops.pack_stem3, layers.FusedStem3, lsmodels.RecNextStem after models.use_fused_stem): the symbols, the
support query and the argument errors that come before any HIP call, the pack layouts, and the reroute's bookkeeping (count, state_dict keys, unchanged CPU
forward).  Reference: lsnet/model/recattn.py:208-223."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn

from recnext_amd import _lib, lsmodels, models, ops
from recnext_amd.layers import FusedStem3
from tests.ls_eager import eager_token_mixer
from tests.test_ls_share_cpu import NAMES as SHARE_NAMES
from tests.test_lsnet_cpu import NAMES, _tiny
from tests.util import GOLDEN

ENTRIES = ("rcx_stem3_supported", "rcx_stem3_pack_bytes", "rcx_stem3_workspace_bytes", "rcx_stem3_fwd")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


def test_header_binding_and_library_agree_on_the_symbols(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "recnext_amd.h")) as f:
        header = f.read()
    for s in ENTRIES:
        assert hasattr(raw, s) and s in _lib.SIGNATURES and s + "(" in header, s
    assert "lsnet/model/recattn.py:208-223" in header
    assert lib.rcx_abi_version() == _lib.ABI_VERSION == 7                      # additions only


def test_queries(lib):
    q = lib.rcx_stem3_supported
    for c in (64, 128):
        for act in (0, 1):
            for n, h, w in ((1, 224, 224), (256, 224, 224), (1, 1, 1), (3, 37, 51), (2, 512, 384)):
                assert q(n, h, w, c, act, 1) == 1, (n, h, w, c, act)
            assert q(1, 224, 224, c, act, 0) == 0 and q(1, 224, 224, c, act, 2) == 0 and q(1, 224, 224, c, act, 9) == 0      # float32, fp16, unknown
        assert q(1, 224, 224, c, 2, 1) == 0 and q(0, 224, 224, c, 1, 1) == 0 and q(1, 0, 224, c, 1, 1) == 0
    for c in (0, 16, 32, 96, 192, 256):
        assert q(1, 224, 224, c, 1, 1) == 0
    assert [lib.rcx_stem3_pack_bytes(64, k) for k in (1, 2, 3)] == [2048, 9 * 1024, 2 * 18 * 1024]
    assert [lib.rcx_stem3_pack_bytes(128, k) for k in (1, 2, 3)] == [2048, 2 * 18 * 1024, 4 * 36 * 1024]
    assert lib.rcx_stem3_pack_bytes(96, 3) == 0 and lib.rcx_stem3_pack_bytes(128, 4) == 0
    assert lib.rcx_stem3_workspace_bytes(256, 224, 224, 128) == 256 * 56 * 56 * 64 * 2
    assert lib.rcx_stem3_workspace_bytes(1, 37, 51, 64) == 10 * 13 * 32 * 2
    assert lib.rcx_stem3_workspace_bytes(1, 37, 51, 96) == 0
    assert ops.stem3_supported(4, 224, 224, 128, False, torch.bfloat16) and not ops.stem3_supported(4, 224, 224, 128, False, torch.float32)


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(1 << 20 << i) for i in range(9)]                    # x, y, six packs, workspace: distinct, aligned, far apart, never dereferenced
    fwd = lib.rcx_stem3_fwd
    need = lib.rcx_stem3_workspace_bytes(1, 16, 16, 64)
    shape = (1, 16, 16, 64, 1, 1)
    for i in range(9):
        args = list(p)
        args[i] = None
        assert fwd(*args, need, *shape, None) == _lib.ERR_BAD_ARG, i
        assert b"null" in lib.rcx_last_error()
    for i in range(1, 9):                                                    # everything but x: 16-byte aligned
        args = list(p)
        args[i] = ctypes.c_void_p(p[i].value + 8)
        assert fwd(*args, need, *shape, None) == _lib.ERR_BAD_ARG, i
        assert b"aligned" in lib.rcx_last_error()
    assert fwd(ctypes.c_void_p(p[0].value + 1), *p[1:], need, *shape, None) == _lib.ERR_BAD_ARG          # half an element
    assert fwd(*p, need, 0, 16, 16, 64, 1, 1, None) == _lib.ERR_BAD_ARG
    assert fwd(*p, need, 1, 16, -1, 64, 1, 1, None) == _lib.ERR_BAD_ARG
    assert fwd(*p, need, 1, 16, 16, 64, 1, 7, None) == _lib.ERR_BAD_ARG                                   # dtype
    assert fwd(*p, need, 1, 16, 16, 64, 3, 1, None) == _lib.ERR_BAD_ARG                                   # final_act
    assert fwd(p[0], p[0], *p[2:], need, *shape, None) == _lib.ERR_BAD_ARG                                # y aliases x
    assert b"overlap" in lib.rcx_last_error()
    assert fwd(*p[:8], p[0], need, *shape, None) == _lib.ERR_BAD_ARG                                      # the workspace aliases x
    assert fwd(*p[:8], ctypes.c_void_p(p[1].value + 16), need, *shape, None) == _lib.ERR_BAD_ARG          # the workspace inside y
    assert fwd(*p, need, 1, 16, 16, 96, 1, 1, None) == _lib.ERR_UNSUPPORTED
    assert fwd(*p, need, 1, 16, 16, 64, 1, 0, None) == _lib.ERR_UNSUPPORTED                               # float32
    assert fwd(*p, need - 1, *shape, None) == _lib.ERR_WORKSPACE
    assert fwd(*p, 0, *shape, None) == _lib.ERR_WORKSPACE


def test_pack_stem3_is_the_fragment_order():
    """As tests/test_models.py does for pack_stem: the layouts against a direct restatement of which lane holds which weight."""
    for c in (64, 128):
        c1, c2 = c // 4, c // 2
        w1 = (torch.arange(c1 * 27, dtype=torch.float32).reshape(c1, 3, 3, 3) * 5) % 127
        w2 = (torch.arange(c2 * c1 * 9, dtype=torch.float32).reshape(c2, c1, 3, 3) * 3) % 113
        w3 = (torch.arange(c * c2 * 9, dtype=torch.float32).reshape(c, c2, 3, 3) * 7) % 109
        b = [torch.arange(k, dtype=torch.float32) - 3 for k in (c1, c2, c)]
        w1p, b1p, w2f, b2p, w3f, b3p = ops.pack_stem3(w1, b[0], w2, b[1], w3, b[2])
        kg2, kg3, mt2, mt3 = c1 // 16, c2 // 16, c2 // 32, c // 32
        assert [t.numel() * t.element_size() for t in (w1p, w2f, w3f)] == [2048, mt2 * 9 * kg2 * 1024, mt3 * 9 * kg3 * 1024]
        assert all(t.dtype == torch.bfloat16 for t in (w1p, w2f, w3f)) and all(t.dtype == torch.float32 for t in (b1p, b2p, b3p))
        assert b1p.numel() == 32 and b2p.numel() == c2 and b3p.numel() == c
        assert torch.equal(b1p[:c1], b[0]) and b1p[c1:].abs().sum() == 0 and torch.equal(b2p, b[1]) and torch.equal(b3p, b[2])
        f1 = w1p.float().view(2, 64, 8)                             # [ks][lane (h, m)][j] = w1[m][k = 16 ks + 8 h + j], k = (dy 3 + dx) 3 + c
        for ks in range(2):
            for lane in range(64):
                for j in range(8):
                    m, k = lane % 32, 16 * ks + 8 * (lane // 32) + j
                    assert f1[ks, lane, j] == (w1[m, k % 3, k // 9, (k // 3) % 3] if m < c1 and k < 27 else 0)
        for f, wt, kg, mts in ((w2f, w2, kg2, mt2), (w3f, w3, kg3, mt3)):
            f = f.float().view(mts, 9 * kg, 64, 8)                  # [mt][ks = tap KG + cg][lane (h, m)][j] = w[32 mt + m][16 cg + 8 h + j][tap]
            want = torch.empty_like(f)
            for ks in range(9 * kg):
                tap, cg = ks // kg, ks % kg
                for hh in range(2):
                    blk = wt[:, 16 * cg + 8 * hh:16 * cg + 8 * hh + 8, tap // 3, tap % 3]              # [co][j]
                    want[:, ks, 32 * hh:32 * hh + 32, :] = blk.view(mts, 32, 8)
            assert torch.equal(f, want)
    with pytest.raises(ValueError):
        ops.pack_stem3(w1, b[0], w2, b[1], w3[:, :-1], b[2])
    with pytest.raises(ValueError):
        ops.pack_stem3(w1[:, :2], b[0], w2, b[1], w3, b[2])


@pytest.mark.parametrize("name", tuple(NAMES) + tuple(SHARE_NAMES))
def test_use_fused_stem_counts_and_keeps_the_keys(name):
    net = models.create_model(name).eval()
    assert models.use_fused_stem(net) == 0                                     # ConvNorm pairs: nothing to run before replace_batchnorm
    models.replace_batchnorm(net)
    keys = list(net.state_dict())
    assert models.use_fused_stem(net) == 1 and models.use_fused_stem(net) == 0
    assert list(net.state_dict()) == keys
    fused = net.stem.__dict__["_fused_stem"]
    assert isinstance(fused, FusedStem3) and fused.final_act == (not name.startswith("recnext_b")) and fused.packs() == []
    assert [m.out_channels for m in fused.convs] == ([16, 32, 64] if name.startswith("recnext_t") else [32, 64, 128])
    x = torch.randn(1, 3, 32, 32)
    assert not fused.supported(x) and not fused.usable(net.stem.stem, x)       # a CPU tensor
    with torch.no_grad():
        want = net.stem.stem(x)
        assert torch.equal(net.stem(x), want)


def test_cpu_forward_is_bit_identical_with_and_without_the_attachment():
    torch.manual_seed(0)
    net = _tiny(eager_token_mixer)
    models.replace_batchnorm(net)
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        want = net(x)
        assert models.use_fused_stem(net) == 1
        assert torch.equal(net(x), want)


def test_usable_follows_replaced_layers_and_gradients(monkeypatch):
    monkeypatch.setattr(FusedStem3, "supported", lambda self, x: True)          # isolate the checks from "is there a kernel on this device"
    net = models.replace_batchnorm(models.create_model("recnext_b").eval())
    models.use_fused_stem(net)
    stem, x = net.stem, torch.randn(1, 3, 32, 32).contiguous(memory_format=torch.channels_last)
    for p in net.parameters():
        p.requires_grad_(False)
    fused = stem._fused_stem
    assert fused.usable(stem.stem, x)
    assert not fused.usable(stem.stem, x.clone().requires_grad_(True))
    assert not fused.usable(stem.stem, torch.randn(2, 3, 32, 32))               # not channels_last
    stem.stem[0].weight.requires_grad_(True)
    assert not fused.usable(stem.stem, x)
    with torch.no_grad():
        assert fused.usable(stem.stem, x)
    stem.stem[0].weight.requires_grad_(False)
    for i, repl in ((1, nn.ReLU()), (3, nn.GELU(approximate="tanh")), (5, nn.GELU()), (2, nn.Conv2d(32, 64, 3, 2, 1))):
        old = stem.stem[i]
        stem.stem[i] = repl
        assert not fused.usable(stem.stem, x), i
        stem.stem[i] = old
        assert fused.usable(stem.stem, x)
    net.train()
    seen = []
    monkeypatch.setattr(FusedStem3, "__call__", lambda self, x: seen.append(1))
    net.stem(x)                                                                 # training mode: the library path whatever usable() says
    assert not seen
