"""CPU: the HIP BatchNorm's interface without a GPU (rcx_batchnorm_*, recnext_amd/batchnorm.py, models.use_hip_batchnorm): the declarations, the
refusals that come before any HIP call, the router, and the float64 reference and bounds of tests/bn64.py held against torch.native_batch_norm in
float32 on the CPU, which shows the reference alone stays inside the bounds."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn as nn

from recnext_amd import _lib, batchnorm, lsmodels, lsshare, models, ops
from tests import bn64
from tests.util import GOLDEN

ROOT = os.path.join(os.path.dirname(GOLDEN), "..")
ENTRIES = ("rcx_batchnorm_supported", "rcx_batchnorm_workspace_bytes", "rcx_batchnorm_train_fwd", "rcx_batchnorm_frozen_fwd", "rcx_batchnorm_bwd")


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


def test_header_library_and_binding_have_the_entries(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "recnext_amd.h")).read()
    for s in ENTRIES:
        assert hasattr(raw, s) and s in _lib.SIGNATURES and s + "(" in header, s
    assert lib.rcx_abi_version() == _lib.ABI_VERSION == 7                      # additions only
    doc = header[header.index("nn.BatchNorm2d of the training step"):header.index("int rcx_batchnorm_supported(")]
    assert "lsnet/model/recattn.py:130-146" in doc and "engine.py:38-71" in doc
    for f in ("batch_norm_supported", "batch_norm_train", "batch_norm_frozen", "batch_norm_backward", "BatchNormFn"):
        assert getattr(ops, f) is getattr(batchnorm, f) and getattr(ops, f).__module__ == "recnext_amd.batchnorm", f
    makefile = open(os.path.join(ROOT, "recnext_amd", "csrc", "Makefile")).read()
    tus = [l for l in makefile.splitlines() if l.startswith("SCRATCH_TUS")][0]
    assert "rcx_bn" in tus.split()


def test_supported_and_workspace_queries(lib):
    sup, q = lib.rcx_batchnorm_supported, lib.rcx_batchnorm_workspace_bytes
    for n, c, h, w in bn64.SHAPES + [bn64.UNALIGNED]:
        for dt in (0, 1, 2):
            assert sup(n, h, w, c, dt) == 1
            a = q(n, h, w, c, dt)
            assert a > 0 and a % (4 * c) == 0 and a == q(n, h, w, c, dt), (n, c, h, w, dt)
            assert 1 <= (a // (4 * c) - 2) // 2 <= 2048                         # P partials of two rows of C floats, and the two rows of sums
    for bad in ((0, 7, 7, 8, 1), (2, 0, 7, 8, 1), (2, 7, -1, 8, 1), (2, 7, 7, 0, 1), (2, 7, 7, 8, 3), (2, 7, 7, 8, -1)):
        assert sup(*bad) == 0 and q(*bad) == 0, bad
    assert sup(1, 1 << 15, 1 << 15, 1, 1) == 1 and sup(1, 1 << 15, 1 << 15, 2, 1) == 0          # 2^30 elements, 2^31 elements
    assert sup(1 << 20, 1 << 20, 1, 1, 0) == 0 and sup(2047, 1 << 10, 1 << 10, 1, 0) == 1
    assert ops.batch_norm_supported(2, 7, 7, 8, torch.bfloat16, measured_only=False) and not ops.batch_norm_supported(2, 7, 7, 8, torch.float64, measured_only=False)


def test_routing_rule_is_a_rule_on_rows_channels_and_element_size():
    """The shapes profiles/r20_batchnorm.txt found faster than the library's BatchNorm at batch 128, from half to twice their rows; nothing else."""
    bf, hf, f32 = torch.bfloat16, torch.float16, torch.float32
    for n in (64, 128, 256):
        assert ops.batch_norm_supported(n, 28, 28, 128, bf) and ops.batch_norm_supported(n, 14, 14, 256, bf) and ops.batch_norm_supported(n, 14, 14, 256, hf)
        assert ops.batch_norm_supported(n, 14, 14, 256, f32) and ops.batch_norm_supported(n, 7, 7, 768, bf)
        assert ops.batch_norm_routed(n, 28, 28, 128, bf) and ops.batch_norm_routed(n * 4, 14, 14, 128, hf)          # R = N H W alone
    for shape in ((128, 112, 112, 32, bf), (128, 28, 28, 128, f32), (128, 14, 14, 512, bf), (128, 4, 4, 512, f32), (128, 7, 7, 768, f32), (32, 14, 14, 256, bf),
                  (512, 14, 14, 256, bf), (2, 7, 7, 8, bf), (128, 14, 14, 256, torch.float64)):
        assert not ops.batch_norm_supported(*shape), shape
    assert ops.batch_norm_supported(2, 7, 7, 8, bf, measured_only=False)


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(1 << 20 | (i + 1) << 14) for i in range(10)]         # distinct, aligned, 16 KiB apart, never dereferenced
    x, y, w, b, rm, rv, sm, si, ws, gy = p
    n, h, wd, c, dt = 2, 7, 7, 16, 1
    need = lib.rcx_batchnorm_workspace_bytes(n, h, wd, c, dt)
    assert 0 < need <= 1 << 14
    BAD, UNS, WS = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    off = lambda q, k: ctypes.c_void_p(q.value + k)

    def train(x=x, y=y, w=w, b=b, rm=rm, rv=rv, sm=sm, si=si, ws=ws, nbytes=need, n=n, h=h, wd=wd, c=c, dt=dt):
        return lib.rcx_batchnorm_train_fwd(x, y, w, b, rm, rv, sm, si, ws, nbytes, n, h, wd, c, 0.1, 1e-5, dt, None)

    for k in ("x", "y", "w", "b", "sm", "si"):
        assert train(**{k: None}) == BAD, k
        assert b"null" in lib.rcx_last_error()
    assert train(rm=None) == BAD and train(rv=None) == BAD                     # one running pointer without the other
    assert b"together" in lib.rcx_last_error()
    assert train(n=0) == BAD and train(h=-1) == BAD and train(c=0) == BAD
    assert train(n=1, h=1, wd=1) == BAD                                        # R = 1 with batch statistics
    assert b"more than one value" in lib.rcx_last_error()
    assert train(dt=5) == BAD
    assert b"dtype" in lib.rcx_last_error()
    for k, v in (("x", off(x, 1)), ("y", off(y, 1)), ("w", off(w, 2)), ("b", off(b, 2)), ("rm", off(rm, 1)), ("sm", off(sm, 2)), ("si", off(si, 3)), ("ws", off(ws, 2))):
        assert train(**{k: v}) == BAD, k
        assert b"aligned" in lib.rcx_last_error()
    for k, v in (("y", x), ("y", off(x, 2 * (n * h * wd * c - 1))), ("sm", w), ("si", sm), ("rm", b), ("rv", rm), ("ws", x), ("ws", off(y, 64)), ("si", off(ws, need - 4)), ("y", off(sm, 4 * (c - 1)))):
        assert train(**{k: v}) == BAD, k                                       # an output or the workspace overlaps an input or another output
        assert b"alias" in lib.rcx_last_error()
    assert train(n=1, h=1 << 15, wd=1 << 15, c=2) == UNS                        # 2^31 elements
    assert b"2^31" in lib.rcx_last_error()
    assert train(nbytes=need - 1) == WS and train(ws=None, nbytes=0) == WS
    assert b"workspace" in lib.rcx_last_error()

    def frozen(x=x, y=y, w=w, b=b, mean=rm, var=rv, si=si, n=n, c=c, dt=dt):
        return lib.rcx_batchnorm_frozen_fwd(x, y, w, b, mean, var, si, 1e-5, n, h, wd, c, dt, None)

    for k in ("x", "y", "w", "b", "mean", "var"):
        assert frozen(**{k: None}) == BAD, k
    assert frozen(n=0) == BAD and frozen(dt=-1) == BAD and frozen(x=off(x, 1)) == BAD and frozen(var=off(rv, 2)) == BAD
    assert frozen(y=x) == BAD and frozen(si=rv) == BAD and frozen(y=off(rm, 8)) == BAD
    assert lib.rcx_batchnorm_frozen_fwd(x, y, w, b, rm, rv, si, 1e-5, 1, 1 << 15, 1 << 15, 2, dt, None) == UNS

    def bwd(x=x, gy=gy, w=w, mean=sm, invstd=si, gx=y, gw=rm, gb=rv, ws=ws, nbytes=need, n=n, h=h, wd=wd, c=c, batch=1, dt=dt):
        return lib.rcx_batchnorm_bwd(x, gy, w, mean, invstd, gx, gw, gb, ws, nbytes, n, h, wd, c, batch, dt, None)

    for k in ("x", "gy", "w", "mean", "invstd"):
        assert bwd(**{k: None}) == BAD, k
    assert bwd(gx=None, gw=None, gb=None) == BAD
    assert b"every output" in lib.rcx_last_error()
    assert bwd(gw=None) == BAD and bwd(gb=None) == BAD                         # the pair comes together
    assert bwd(batch=2) == BAD and bwd(n=0) == BAD and bwd(dt=3) == BAD and bwd(n=1, h=1, wd=1) == BAD
    assert bwd(gy=off(gy, 1)) == BAD and bwd(gx=off(y, 1)) == BAD and bwd(gw=off(rm, 2)) == BAD and bwd(ws=off(ws, 1)) == BAD
    for k, v in (("gx", x), ("gx", gy), ("gw", w), ("gb", sm), ("gb", rm), ("ws", si), ("ws", y), ("gx", off(ws, 8))):
        assert bwd(**{k: v}) == BAD, k
        assert b"alias" in lib.rcx_last_error()
    assert bwd(n=1, h=1 << 15, wd=1 << 15, c=2) == UNS
    assert bwd(nbytes=need - 1) == WS and bwd(ws=None, nbytes=0) == WS
    assert bwd(batch=0, nbytes=need - 1) == WS                                  # frozen with the pair still reduces
    assert bwd(batch=0, gx=None, ws=None, nbytes=0) == WS


def test_functions_refuse_bad_arguments_and_cpu_tensors():
    x = torch.randn(2, 8, 3, 3).contiguous(memory_format=torch.channels_last)
    w, b = torch.ones(8), torch.zeros(8)
    with pytest.raises(_lib.RcxError):
        ops.batch_norm_train(x, w, b)
    with pytest.raises(ValueError):
        ops.batch_norm_train(x[0], w, b)
    with pytest.raises(ValueError):
        ops.batch_norm_train(x.double(), w, b)
    with pytest.raises(ValueError):
        ops.batch_norm_frozen(x[0], w, b, b, w)
    with pytest.raises(ValueError):
        ops.batch_norm_backward(x[0], x, w, b, w)
    with pytest.raises(_lib.RcxError):
        ops.BatchNormFn.apply(x.requires_grad_(True), w, b, None, None, True, 0.1, 1e-5)


# ---- the router ---------------------------------------------------------------------------------------------------------------------------------------------

_LS_TINY = dict(embed_dim=(32, 64, 96, 128), depth=(1, 1, 2, 2), mlp_ratios=(2, 2, 2, 1.5), split_rates=(4, 4, 4, 4), num_classes=10)


def _builders():
    """Tiny models of the three model modules, their token mixers on library operators so that they run on the CPU."""
    from tests.ls_eager import eager_token_mixer
    from tests.ls_share_eager import eager_share_token_mixer
    return {
        "models": lambda: models.RecNext(family="m", embed_dim=(8, 16, 32, 64), depth=(1, 1, 1, 1), num_classes=10,
                                         token_mixer=lambda dim, stage: nn.Conv2d(dim, dim, 3, padding=1, groups=dim)),
        "lsmodels": lambda: lsmodels.RecNext(token_mixer=eager_token_mixer, num_heads=(1, 1, 1, 2), **_LS_TINY),
        "lsshare": lambda: lsshare.RecNext(token_mixer=eager_share_token_mixer, **dict(_LS_TINY, depth=(1, 1, 2, 6))),
    }


@pytest.mark.parametrize("which", ["models", "lsmodels", "lsshare"])
def test_router_keeps_keys_tensors_and_parameter_objects(which):
    torch.manual_seed(1)
    net = _builders()[which]()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    params = {k: id(p) for k, p in net.named_parameters()}
    buffers = {k: id(b) for k, b in net.named_buffers()}
    mods = {k: id(m) for k, m in net.named_modules()}
    plain = sum(type(m) is nn.BatchNorm2d for m in net.modules())
    assert plain > 0
    assert models.use_hip_batchnorm(net, all_shapes=(which == "lsshare")) == plain
    assert all(m.hip_all_shapes == (which == "lsshare") for m in net.modules() if type(m) is batchnorm.HipBatchNorm2d)
    assert models.use_hip_batchnorm(net) == 0                                   # idempotent
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert {k: id(p) for k, p in net.named_parameters()} == params and {k: id(b) for k, b in net.named_buffers()} == buffers
    assert {k: id(m) for k, m in net.named_modules()} == mods                  # module identity survives
    assert not any(type(m) is nn.BatchNorm2d for m in net.modules())
    assert all(isinstance(m, nn.BatchNorm2d) for m in net.modules() if type(m) is batchnorm.HipBatchNorm2d)
    # strict loads both ways
    fresh = _builders()[which]()
    fresh.load_state_dict(net.state_dict(), strict=True)
    net.load_state_dict(fresh.state_dict(), strict=True)
    # SyncBatchNorm still converts the new modules
    sync = nn.SyncBatchNorm.convert_sync_batchnorm(copy.deepcopy(net))
    assert sum(isinstance(m, nn.SyncBatchNorm) for m in sync.modules()) >= plain


def test_rerouted_tiny_model_equals_the_unrouted_one_on_the_cpu():
    torch.manual_seed(2)
    ref = _builders()["lsmodels"]()
    hip = copy.deepcopy(ref)
    assert models.use_hip_batchnorm(hip) > 0
    x = torch.randn(2, 3, 64, 64)
    y = torch.tensor([1, 7])
    for net in (ref, hip):
        net.train()
        nn.functional.cross_entropy(net(x), y).backward()
    for (k, p), (_, q) in zip(ref.named_parameters(), hip.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    for (k, a), (_, b) in zip(ref.named_buffers(), hip.named_buffers()):
        assert torch.equal(a, b), k
    ref.eval(), hip.eval()
    with torch.no_grad():
        assert torch.equal(ref(x), hip(x))
    assert torch.equal(ref(x), hip(x))                                         # eval with gradients on, on the CPU: the parent's forward too


# ---- the reference and its bounds, against ATen's float32 BatchNorm ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dist", bn64.DISTS)
@pytest.mark.parametrize("shape", bn64.SHAPES + [bn64.UNALIGNED], ids=lambda s: "x".join(map(str, s)))
def test_reference_bounds_hold_for_aten_float32(shape, dist, record_property):
    d = bn64.case(shape, torch.float32, dist)
    x, gy, w, b = d["x"], d["gy"], d["weight"], d["bias"]
    f32 = torch.float32
    worst = {}
    rm, rv = d["running_mean"].clone(), d["running_var"].clone()
    y, mean, invstd = torch.native_batch_norm(x, w, b, rm, rv, True, bn64.MOMENTUM, bn64.EPS)
    ref = bn64.forward_ref(x, w, b, bn64.EPS, running_mean=d["running_mean"], running_var=d["running_var"])
    for name, got in (("y", y), ("save_mean", mean), ("save_invstd", invstd), ("running_mean", rm), ("running_var", rv)):
        worst[name] = bn64.check(got, ref[name], f32, name)
    gx, gw, gb = torch.ops.aten.native_batch_norm_backward(gy, x, w, rm, rv, mean, invstd, True, bn64.EPS, [True, True, True])
    refb = bn64.backward_ref(x, gy, w, mean, invstd, True)
    for name, got in (("gx", gx), ("gweight", gw), ("gbias", gb)):
        worst[name] = bn64.check(got, refb[name], f32, name)
    # frozen statistics
    yf, _, _ = torch.native_batch_norm(x, w, b, d["running_mean"], d["running_var"], False, bn64.MOMENTUM, bn64.EPS)
    worst["y_frozen"] = bn64.check(yf, bn64.forward_ref(x, w, b, bn64.EPS, mean=d["running_mean"], var=d["running_var"])["y"], f32, "frozen y")
    inv = (1.0 / torch.sqrt(d["running_var"].double() + float(torch.tensor(bn64.EPS)))).float()
    gxf, gwf, gbf = torch.ops.aten.native_batch_norm_backward(gy, x, w, d["running_mean"], d["running_var"], None, None, False, bn64.EPS, [True, True, True])
    reff = bn64.backward_ref(x, gy, w, d["running_mean"], inv, False)
    for name, got in (("gx", gxf), ("gweight", gwf), ("gbias", gbf)):
        worst[name + "_frozen"] = bn64.check(got, reff[name], f32, "frozen " + name)
    record_property("worst_ratio", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 24.0
