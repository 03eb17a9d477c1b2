"""CPU: the wide linear-attention core's C entries (rcx_linear_attention_wide_*: declared, exported, argument checks, the support query) and the
training semantics of tests/ls_eager.py pinned to the reference itself by tests/golden/ls_grad_*.npz (train mode, float64)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from recnext_amd import _lib, lsmodels
from tests.ls_eager import eager_token_mixer, token_half

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
WIDE = ("rcx_linear_attention_wide_supported", "rcx_linear_attention_wide_fwd", "rcx_linear_attention_wide_bwd")
GRAD_NAMES = ["s0_28x28_c32", "s1_14x14_c128", "s1_9x9_c256", "s2_7x7_c256", "s2_7x7_c384", "s3_4x4_c512"]   # tests/golden/make_golden_ls_grad.py ROWS


def _bf16(a):
    return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).double()


def load_grad_case(name):
    """(x, gy, sd, t, gx, grads, running, meta) of tests/golden/ls_grad_<name>.npz; tensors float64 on the CPU."""
    d = np.load(os.path.join(GOLDEN, f"ls_grad_{name}.npz"))
    meta = json.loads(str(d["meta"]))
    pick = lambda pre: {k[len(pre):]: torch.from_numpy(d[k]).double() for k in d.files if k.startswith(pre)}
    return (_bf16(d["x_bf16"]), _bf16(d["gy_bf16"]), pick("sd::"), torch.from_numpy(d["t"]).double(), torch.from_numpy(d["gx"]).double(),
            pick("grad::"), pick("run::"), meta)


def build_train_block(meta, sd, token_mixer=None):
    """An lsmodels.MetaNeXtBlock in train mode with the fixture's rep_mixer / token_mixer state (the channel mixer keeps its initialisation)."""
    blk = lsmodels.MetaNeXtBlock(meta["C"], meta["mlp_ratio"], num_heads=meta["num_heads"], stage=meta["stage"], token_mixer=token_mixer)
    missing, unexpected = blk.load_state_dict({k: v.float() for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.startswith("channel_mixer.") for k in missing), (missing, unexpected)
    return blk.train()


def _declared():
    src = open(os.path.join(ROOT, "include", "recnext_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", src))


def test_wide_entries_declared_and_exported():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in WIDE:
        assert name in _declared(), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().rcx_abi_version() == 7


def test_wide_entries_reject_bad_arguments_before_device_work():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    fwd = lambda *a: lib.rcx_linear_attention_wide_fwd(*a, None)
    bwd = lambda *a: lib.rcx_linear_attention_wide_bwd(*a, None)
    ok = (2, 16, 64, 128, 1, 0)
    assert fwd(None, p, p, p, p, *ok) == _lib.ERR_BAD_ARG
    assert fwd(p, p, p, p, None, *ok) == _lib.ERR_BAD_ARG
    assert bwd(p, p, p, p, p, p, None, *ok) == _lib.ERR_BAD_ARG
    for bad in [(0, 16, 64, 128, 1, 0), (2, 0, 64, 128, 1, 0), (2, 16, -64, 128, 1, 0), (2, 16, 64, 128, 0, 0), (2, 16, 64, 128, 1, 7),
                (2, 16, 64, 126, 4, 0)]:                                 # 126 channels in 4 heads: heads do not divide Cv
        assert fwd(p, p, p, p, p, *bad) == _lib.ERR_BAD_ARG, bad
        assert bwd(p, p, p, p, p, p, p, *bad) == _lib.ERR_BAD_ARG, bad
    assert fwd(p + 4, p, p, p, p, *ok) == _lib.ERR_BAD_ARG                   # float32 tensors aligned to 16 bytes
    assert fwd(p + 2, p, p, p, p, 2, 16, 64, 128, 1, 1) == _lib.ERR_BAD_ARG  # bf16: 8 bytes
    assert "aligned" in lib.rcx_last_error().decode()
    assert fwd(p, p, p, p, p, 2, 16, 64, 136, 1, 0) == _lib.ERR_UNSUPPORTED  # Dv 136 > 128
    assert bwd(p, p, p, p, p, p, p, 2, 16, 66, 128, 1, 0) == _lib.ERR_UNSUPPORTED


def test_wide_support_query():
    q = _lib.load().rcx_linear_attention_wide_supported
    # the table's shapes (B, n, Cqk, Cv, heads) and the 384 x 384 planes, every dtype
    for dt in (0, 1, 2):
        for args in [(128, 16, 96, 96, 1), (128, 16, 64, 128, 1), (2, 36, 96, 96, 1), (2, 36, 64, 128, 1), (2, 196, 32, 32, 1), (2, 49, 64, 64, 1),
                     (4, 576, 32, 64, 1), (4, 45, 256, 128, 2), (2, 1, 4, 4, 1), (3, 16, 256, 256, 2), (1, 5000, 128, 128, 1)]:
            assert q(*args, dt) == 1, (args, dt)
    for args in [(2, 16, 98, 96, 1),       # Dk not a multiple of 4
                 (2, 16, 96, 90, 1),       # Dv not a multiple of 4
                 (2, 16, 132, 64, 1),      # Dk above 128
                 (2, 16, 64, 132, 1),      # Dv above 128
                 (2, 16, 512, 512, 2),     # 256-wide heads: above 128 and above the LDS budget
                 (2, 16, 96, 96, 5), (0, 16, 96, 96, 1), (2, 0, 96, 96, 1), (2, 16, 96, 96, 0)]:
        assert q(*args, 0) == 0, args
    assert q(2, 16, 96, 96, 1, 3) == 0


@pytest.mark.parametrize("name", GRAD_NAMES)
def test_eager_training_matches_reference_fixture(name):
    """tests/ls_eager.py's operator chain in train mode, float64: t, dL/dx, every parameter gradient and the running statistics after the step."""
    x, gy, sd, t_ref, gx_ref, grads, running, meta = load_grad_case(name)
    blk = build_train_block(meta, sd, token_mixer=eager_token_mixer).double()
    x = x.clone().requires_grad_()
    _, t = token_half(blk, x)
    (t * gy).sum().backward()
    # relative to the tensor's largest entry, with an absolute floor: a conv bias in front of a train-mode BatchNorm has a zero gradient
    # (the batch mean removes it), which both sides give as float64 rounding noise
    rel = lambda a, b: float((a - b).abs().max()) / max(1e-6, float(b.abs().max()))
    assert rel(t.detach(), t_ref) < 1e-6
    assert rel(x.grad, gx_ref) < 1e-6
    params = dict(blk.named_parameters())
    assert set(grads) == {k for k in params if not k.startswith("channel_mixer.")}
    for k, g in grads.items():
        assert rel(params[k].grad, g) < 1e-5, k
    state = blk.state_dict()
    assert running
    for k, v in running.items():
        assert rel(state[k], v) < 1e-12, k


def test_cpu_training_forward_still_raises():
    _, _, sd, _, _, _, _, meta = load_grad_case("s3_4x4_c512")
    blk = build_train_block(meta, sd)
    with pytest.raises(NotImplementedError, match="training"):
        blk(torch.randn(2, meta["C"], 4, 4))
