"""CPU: the one-operator RepVGGDW's interface without a GPU (rcx_repdw_train_*, recnext_amd/repdw.py, models.use_fused_rep_train): the declarations, the
queries, the refusals that come before any HIP call, the router, and the float64 reference and bounds of tests/rep64.py held against the operator chain
on ATen in float32 on the CPU (F.conv2d, F.batch_norm(training=True), autograd), which shows the library's own operators stay inside the bounds."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from recnext_amd import _lib, lsmodels, models, ops, repdw
from tests import bn64, rep64
from tests.test_batchnorm_cpu import _builders
from tests.util import GOLDEN

ROOT = os.path.join(os.path.dirname(GOLDEN), "..")
ENTRIES = ("rcx_repdw_train_supported", "rcx_repdw_train_workspace_bytes", "rcx_repdw_train_fwd", "rcx_repdw_train_bwd")


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
    doc = header[header.index("RepVGGDW of the training step as one operator"):header.index("int rcx_repdw_train_supported(")]
    assert "lsnet/model/recattn.py:8-15" in doc
    for f in ("repdw_train_supported", "repdw_train", "repdw_train_backward", "RepDwFn"):
        assert getattr(ops, f) is getattr(repdw, f) and getattr(ops, f).__module__ == "recnext_amd.repdw", f
    makefile = open(os.path.join(ROOT, "recnext_amd", "csrc", "Makefile")).read()
    tus = [l for l in makefile.splitlines() if l.startswith("SCRATCH_TUS")][0]
    assert "rcx_repdw" in tus.split()
    assert os.path.exists(os.path.join(ROOT, "recnext_amd", "csrc", "rcx_bn.h"))   # the helpers rcx_bn.hip and rcx_repdw.hip share, in one place
    for tu in ("rcx_bn.hip", "rcx_repdw.hip"):
        src = open(os.path.join(ROOT, "recnext_amd", "csrc", tu)).read()
        assert '#include "rcx_bn.h"' in src and "void chan(" not in src and "atomicAdd" not in src and "__hip_atomic" not in src, tu


def test_supported_and_workspace_queries(lib):
    sup, q = lib.rcx_repdw_train_supported, lib.rcx_repdw_train_workspace_bytes
    for n, c, h, w in rep64.SHAPES + [bn64.UNALIGNED]:
        for dt in (0, 1, 2):
            assert sup(n, h, w, c, dt) == 1
            a = q(n, h, w, c, dt)
            assert a > 0 and a % (4 * c) == 0 and a == q(n, h, w, c, dt), (n, c, h, w, dt)
            assert 1 <= (a // (4 * c) - 3) // 9 <= 2048 and (a // (4 * c) - 3) % 9 == 0     # three rows of sums, then P partials of nine rows of C floats
    for bad in ((0, 7, 7, 8, 1), (2, 0, 7, 8, 1), (2, 7, -1, 8, 1), (2, 7, 7, 0, 1), (2, 7, 7, 8, 3), (2, 7, 7, 8, -1)):
        assert sup(*bad) == 0 and q(*bad) == 0, bad
    assert sup(1, 1 << 15, 1 << 15, 1, 1) == 1 and sup(1, 1 << 15, 1 << 15, 2, 1) == 0          # 2^30 elements, 2^31 elements
    assert ops.repdw_train_supported(2, 7, 7, 8, torch.bfloat16) and not ops.repdw_train_supported(2, 7, 7, 8, torch.float64)
    for (c, es), (lo, hi) in repdw.ROUTED.items():                              # the routing rule: rows, channels and element size alone
        dt = torch.float32 if es == 4 else torch.bfloat16
        assert ops.repdw_train_routed(1, 1, lo, c, dt) and ops.repdw_train_routed(hi, 1, 1, c, dt) and not ops.repdw_train_routed(1, 1, hi + 1, c, dt)
        assert ops.repdw_train_supported(1, lo, 1, c, dt, measured_only=True)
    assert not ops.repdw_train_routed(2, 7, 7, 8, torch.bfloat16) and not ops.repdw_train_supported(2, 7, 7, 8, torch.bfloat16, measured_only=True)


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(1 << 22 | (i + 1) << 14) for i in range(32)]           # distinct, aligned, 16 KiB apart, never dereferenced
    n, h, wd, c, dt = 2, 7, 7, 16, 1
    need = lib.rcx_repdw_train_workspace_bytes(n, h, wd, c, dt)
    assert 0 < need <= 1 << 14
    BAD, UNS, WS = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    off = lambda q, k: ctypes.c_void_p(q.value + k)
    fnames = ("x", "r", "w3", "b3", "ga", "ba", "w1", "b1", "gb", "bb", "lrm", "lrv", "srm", "srv", "mx", "vx", "mu", "ia", "ws")
    base = dict(zip(fnames, p))

    def fwd(nbytes=need, n=n, h=h, wd=wd, c=c, dt=dt, **kw):
        a = dict(base, **kw)
        return lib.rcx_repdw_train_fwd(*[a[k] for k in fnames], nbytes, n, h, wd, c, 0.1, 1e-5, 0.1, 1e-5, dt, None)

    for k in fnames:
        if k not in ("lrm", "lrv", "srm", "srv", "ws"):
            assert fwd(**{k: None}) == BAD, k
            assert b"null" in lib.rcx_last_error()
    for k in ("lrm", "lrv", "srm", "srv"):
        assert fwd(**{k: None}) == BAD, k                                       # a running pointer without its partners
        assert b"together" in lib.rcx_last_error()
    assert fwd(lrm=None, lrv=None) == BAD and fwd(lrm=None, lrv=None, srm=None) == BAD
    assert fwd(n=0) == BAD and fwd(h=-1) == BAD and fwd(wd=0) == BAD and fwd(c=0) == BAD
    assert fwd(n=1, h=1, wd=1) == BAD                                           # R = 1
    assert b"more than one value" in lib.rcx_last_error()
    assert fwd(dt=5) == BAD
    assert b"dtype" in lib.rcx_last_error()
    for k, v in (("x", off(p[0], 1)), ("r", off(p[1], 2)), ("w3", off(p[2], 2)), ("w1", off(p[6], 1)), ("lrm", off(p[10], 2)), ("vx", off(p[15], 3)),
                 ("ws", off(p[18], 2))):
        assert fwd(**{k: v}) == BAD, k
        assert b"aligned" in lib.rcx_last_error()
    xb, rb = 2 * n * h * wd * c, 4 * n * h * wd * c
    for k, v in (("r", base["x"]), ("r", off(base["x"], xb - 4)), ("mx", base["w3"]), ("mx", off(base["w3"], 36 * c - 4)), ("vx", base["mx"]), ("lrm", base["b3"]),
                 ("srv", base["lrm"]), ("ws", base["x"]), ("ws", off(base["r"], 64)), ("ia", off(base["ws"], need - 4)), ("mu", off(base["r"], rb - 4)),
                 ("srm", base["bb"])):
        assert fwd(**{k: v}) == BAD, k                                          # an output or the workspace overlaps an input or another output
        assert b"alias" in lib.rcx_last_error()
    assert fwd(n=1, h=1 << 15, wd=1 << 15, c=2) == UNS                          # 2^31 elements
    assert b"2^31" in lib.rcx_last_error()
    assert fwd(nbytes=need - 1) == WS and fwd(ws=None, nbytes=0) == WS
    assert b"workspace" in lib.rcx_last_error()
    assert fwd(lrm=None, lrv=None, srm=None, srv=None, nbytes=need - 1) == WS   # the quartet may be NULL: the call gets as far as the workspace

    bnames = ("x", "g", "w3", "b3", "ga", "w1", "gb", "mx", "vx", "mu", "ia", "gx", "gw3", "gb3", "gga", "gba", "gw1", "gb1", "ggb", "gbb", "ws")
    bbase = dict(zip(bnames, p))
    grads = bnames[12:20]

    def bwd(nbytes=need, n=n, h=h, wd=wd, c=c, dt=dt, **kw):
        a = dict(bbase, **kw)
        return lib.rcx_repdw_train_bwd(*[a[k] for k in bnames], nbytes, n, h, wd, c, 1e-5, dt, None)

    for k in bnames[:11]:
        assert bwd(**{k: None}) == BAD, k
        assert b"null" in lib.rcx_last_error()
    none = {k: None for k in grads}
    assert bwd(gx=None, **none) == BAD
    assert b"every output" in lib.rcx_last_error()
    for k in grads:
        assert bwd(**{k: None}) == BAD, k                                       # one of the eight alone
        assert b"together" in lib.rcx_last_error()
    assert bwd(n=0) == BAD and bwd(c=-3) == BAD and bwd(dt=3) == BAD and bwd(n=1, h=1, wd=1) == BAD
    assert bwd(x=off(p[0], 1)) == BAD and bwd(g=off(p[1], 2)) == BAD and bwd(gx=off(p[11], 1)) == BAD and bwd(gw1=off(p[16], 2)) == BAD and bwd(ws=off(p[20], 1)) == BAD
    for k, v in (("gx", bbase["x"]), ("gx", bbase["g"]), ("gw3", bbase["w3"]), ("gb3", bbase["mx"]), ("gbb", bbase["gga"]), ("ws", bbase["ia"]), ("ws", bbase["gx"]),
                 ("gx", off(bbase["ws"], 8)), ("gb1", off(bbase["gw3"], 36 * c - 4))):
        assert bwd(**{k: v}) == BAD, k
        assert b"alias" in lib.rcx_last_error()
    assert bwd(n=1, h=1 << 15, wd=1 << 15, c=2) == UNS
    assert bwd(nbytes=need - 1) == WS and bwd(ws=None, nbytes=0) == WS
    assert bwd(gx=None, nbytes=need - 1) == WS and bwd(nbytes=need - 1, **none) == WS      # either half alone is a valid request


def test_functions_refuse_bad_arguments_and_cpu_tensors():
    d = rep64.case((2, 8, 1, 1), torch.float32, "normal")
    x = d["x"].expand(2, 8, 3, 3).contiguous(memory_format=torch.channels_last)
    par = [d[k] for k in rep64.PARAMS]
    with pytest.raises(_lib.RcxError):
        ops.repdw_train(x, *par)
    with pytest.raises(ValueError):
        ops.repdw_train(x[0], *par)
    with pytest.raises(ValueError):
        ops.repdw_train(x.double(), *par)
    with pytest.raises(ValueError):
        ops.repdw_train_backward(x[0], x, d["w3"], d["b3"], d["gamma_a"], d["w1"], d["gamma_b"], torch.zeros(4, 8))
    with pytest.raises(_lib.RcxError):
        ops.RepDwFn.apply(x.requires_grad_(True), *par, None, None, None, None, 0.1, 1e-5, 0.1, 1e-5)


# ---- the router ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["lsmodels", "lsshare"])
def test_router_keeps_keys_tensors_and_parameter_objects(which):
    torch.manual_seed(1)
    net = _builders()[which]()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    params = {k: id(p) for k, p in net.named_parameters()}
    buffers = {k: id(b) for k, b in net.named_buffers()}
    mods = {k: (id(m), type(m)) for k, m in net.named_modules()}
    reps = [m for m in net.modules() if isinstance(m, lsmodels.RepVGGDW)]
    assert reps and not any("_fused_rep_train" in m.__dict__ for m in reps)    # nothing is marked unless asked for
    assert models.use_fused_rep_train(net) == len(reps)
    assert models.use_fused_rep_train(net) == 0 and models.use_fused_rep_train(net, all_shapes=True) == 0        # idempotent
    assert all(m.__dict__["_fused_rep_train"] == "all" for m in reps)
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert {k: id(p) for k, p in net.named_parameters()} == params and {k: id(b) for k, b in net.named_buffers()} == buffers
    assert {k: (id(m), type(m)) for k, m in net.named_modules()} == mods
    fresh = _builders()[which]()
    fresh.load_state_dict(net.state_dict(), strict=True)
    net.load_state_dict(fresh.state_dict(), strict=True)
    assert all(m.__dict__["_fused_rep_train"] == "all" for m in copy.deepcopy(net).modules() if isinstance(m, lsmodels.RepVGGDW))
    assert models.use_fused_rep_train(_builders()["models"]()) == 0             # the M / A families have no RepVGGDW


def test_routed_tiny_model_equals_the_unrouted_one_on_the_cpu():
    torch.manual_seed(2)
    ref = _builders()["lsmodels"]()
    hip = copy.deepcopy(ref)
    assert models.use_fused_rep_train(hip, all_shapes=True) > 0
    x = torch.randn(2, 3, 64, 64)
    y = torch.tensor([1, 7])
    for net in (ref, hip):
        net.train()
        F.cross_entropy(net(x), y).backward()
    for (k, p), (_, q) in zip(ref.named_parameters(), hip.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    for (k, a), (_, b) in zip(ref.named_buffers(), hip.named_buffers()):
        assert torch.equal(a, b), k


# ---- the reference and its bounds, against the operator chain on ATen in float32 --------------------------------------------------------------------------

def aten_chain(d):
    """The unfused RepVGGDW on ATen in float32 with autograd: -> (outputs by rep64's names, the float32 (4, C) statistics the chain itself formed)."""
    c = d["x"].shape[1]
    x = d["x"].clone().requires_grad_(True)
    p = {k: d[k].clone().requires_grad_(True) for k in rep64.PARAMS}
    run = {k: d[k].clone() for k in rep64.RUNNING}
    u = F.conv2d(x, p["w3"], p["b3"], padding=1, groups=c)
    v = F.conv2d(x, p["w1"], p["b1"], groups=c)
    lk = F.batch_norm(u, run["lk_running_mean"], run["lk_running_var"], p["gamma_a"], p["beta_a"], True, rep64.MOM_A, rep64.EPS_A)
    sk = F.batch_norm(v, run["sk_running_mean"], run["sk_running_var"], p["gamma_b"], p["beta_b"], True, rep64.MOM_B, rep64.EPS_B)
    r = lk + sk + x
    grads = torch.autograd.grad(r, [x] + [p[k] for k in rep64.PARAMS], d["g"])
    out = dict(run, r=r.detach(), gx=grads[0])
    out.update({"g" + k: t for k, t in zip(rep64.PARAMS, grads[1:])})
    with torch.no_grad():
        _, mean_u, invstd_u = torch.native_batch_norm(u, None, None, None, None, True, 0.0, rep64.EPS_A)
        var_x, mean_x = torch.var_mean(d["x"], dim=(0, 2, 3), unbiased=False)
    out.update(mean_x=mean_x, var_x=var_x, mean_u=mean_u, invstd_u=invstd_u)
    return out, torch.stack([mean_x, var_x, mean_u, invstd_u])


@pytest.mark.parametrize("dist", bn64.DISTS)
@pytest.mark.parametrize("shape", rep64.SHAPES + [bn64.UNALIGNED], ids=lambda s: "x".join(map(str, s)))
def test_reference_bounds_hold_for_the_aten_chain(shape, dist, record_property):
    d = rep64.case(shape, torch.float32, dist)
    got, stats = aten_chain(d)
    f32 = torch.float32
    worst = {}
    ref = rep64.forward_ref(d["x"], d, running=d)
    for name in ("r",) + rep64.STATS + rep64.RUNNING:
        worst[name] = rep64.check(got[name], ref[name], f32, f"{shape} {dist} {name}")
    refb = rep64.backward_ref(d["x"], d["g"], d, stats)
    for name in ("gx",) + rep64.GRADS:
        worst[name] = rep64.check(got[name], refb[name], f32, f"{shape} {dist} {name}")
    record_property("worst_ratio", {k: round(v, 3) for k, v in worst.items()})
    print(f"  {shape} {dist}: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= 24.0
