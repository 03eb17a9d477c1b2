"""CPU: the one-operator depthwise ConvNorm's interface without a GPU (rcx_dwconv_bn_train_*, recnext_amd/dwbn.py, models.use_fused_conv_norm_train): the
declarations, the queries, the refusals that come before any HIP call, the router, and the float64 reference and bounds of tests/conv64.py held against
the operator chain on ATen in float32 on the CPU (F.interpolate, F.conv2d, F.batch_norm(training=True), autograd), which validates the reference and the
bounds before any kernel is judged by them."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from recnext_amd import _lib, dwbn, lsmodels, models, ops, recattn
from tests import bn64, conv64
from tests.test_batchnorm_cpu import _builders
from tests.util import GOLDEN

ROOT = os.path.join(os.path.dirname(GOLDEN), "..")
ENTRIES = ("rcx_dwconv_bn_train_supported", "rcx_dwconv_bn_train_workspace_bytes", "rcx_dwconv_bn_train_fwd", "rcx_dwconv_bn_train_bwd")
_FORM_IDS = ["k%ds%d%s" % (k, s, "up" if up else "") for k, s, up in conv64.FORMS]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    return _lib.load()


def test_header_library_and_binding_have_the_entries(lib):
    raw = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "recnext_amd.h")).read()
    for s in ENTRIES:
        assert hasattr(raw, s) and s in _lib.SIGNATURES and "int " + s + "(" in header.replace("size_t " + s, "int " + s), s
    doc = header[header.index("A depthwise ConvNorm of the training step as one operator"):header.index("int rcx_dwconv_bn_train_supported(")]
    assert "gb = 0 (exactly" in doc and "u is never formed again" in doc
    for f in ("dwconv_bn_train_supported", "dwconv_bn_train_routed", "dwconv_bn_train", "dwconv_bn_train_backward", "DwConvBnFn"):
        assert getattr(ops, f) is getattr(dwbn, f) and getattr(ops, f).__module__ == "recnext_amd.dwbn", f
    makefile = open(os.path.join(ROOT, "recnext_amd", "csrc", "Makefile")).read()
    tus = [l for l in makefile.splitlines() if l.startswith("SCRATCH_TUS")][0]
    assert "rcx_dwbn" in tus.split()                                            # the no-scratch gate covers the new translation unit
    src = open(os.path.join(ROOT, "recnext_amd", "csrc", "rcx_dwbn.hip")).read()
    assert '#include "rcx_bn.h"' in src and "atomicAdd" not in src and "__hip_atomic" not in src


def test_supported_and_workspace_queries(lib):
    sup, q = lib.rcx_dwconv_bn_train_supported, lib.rcx_dwconv_bn_train_workspace_bytes
    for n, c, h, w in conv64.SHAPES + [bn64.UNALIGNED]:
        for k, stride, up in conv64.FORMS:
            for dt in (0, 1, 2):
                assert sup(n, h, w, c, k, stride, int(up), dt) == 1
                a = q(n, h, w, c, k, stride, int(up), dt)
                assert a > 0 and a % (4 * c) == 0 and a == q(n, h, w, c, k, stride, int(up), dt), (n, c, h, w, k, stride, up, dt)
                assert 1 <= (a // (4 * c) - 2) // (k * k) <= 2048 and (a // (4 * c) - 2) % (k * k) == 0     # two rows of sums, then P partials of k k rows
    assert sup(2, 7, 7, 8, 4, 1, 0, 1) == 0 and q(2, 7, 7, 8, 4, 1, 0, 1) == 0                  # k = 4
    assert sup(2, 7, 7, 8, 7, 1, 0, 1) == 0 and sup(2, 7, 7, 8, 1, 1, 0, 1) == 0
    assert sup(2, 7, 7, 8, 5, 3, 0, 1) == 0 and q(2, 7, 7, 8, 5, 3, 0, 1) == 0                  # stride 3
    assert sup(2, 7, 7, 8, 5, 0, 0, 1) == 0
    assert sup(2, 7, 7, 8, 5, 2, 1, 1) == 0 and q(2, 7, 7, 8, 5, 2, 1, 1) == 0                  # up-add with stride 2
    assert sup(2, 7, 7, 8, 5, 1, 2, 1) == 0
    for bad in ((0, 7, 7, 8), (2, 0, 7, 8), (2, 7, -1, 8), (2, 7, 7, 0)):
        assert sup(*bad, 5, 1, 0, 1) == 0 and q(*bad, 5, 1, 0, 1) == 0, bad
    assert sup(2, 7, 7, 8, 5, 1, 0, 3) == 0 and sup(2, 7, 7, 8, 5, 1, 0, -1) == 0
    assert sup(1, 1 << 15, 1 << 15, 1, 3, 1, 0, 1) == 1 and sup(1, 1 << 15, 1 << 15, 2, 3, 1, 0, 1) == 0        # 2^30 elements, 2^31 elements
    for c in (1, 21, 64, 384):                                                  # positive and monotone in R = N Ho Wo
        for k, stride, up in conv64.FORMS:
            for dt in (0, 1):
                sizes = [q(n, 14, 14, c, k, stride, int(up), dt) for n in (1, 2, 3, 5, 8, 16, 33, 64, 128, 500, 2048, 8192)]
                assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], (c, k, stride, up, dt, sizes)
    assert ops.dwconv_bn_train_supported(2, 7, 7, 8, 5, 2, False, torch.bfloat16) and not ops.dwconv_bn_train_supported(2, 7, 7, 8, 5, 2, True, torch.bfloat16)
    assert not ops.dwconv_bn_train_supported(2, 7, 7, 8, 5, 1, False, torch.float64)
    for (c, k, stride, up, es), (lo, hi) in dwbn.ROUTED.items():                 # the routing rule: output rows, channels, form and element size alone
        dt = torch.float32 if es == 4 else torch.bfloat16
        assert ops.dwconv_bn_train_routed(lo, 1, 1, c, k, stride, up, dt) and ops.dwconv_bn_train_routed(hi, 1, 1, c, k, stride, up, dt)
        assert not ops.dwconv_bn_train_routed(hi + 1, 1, 1, c, k, stride, up, dt) and not ops.dwconv_bn_train_routed(lo, 1, 1, c, 8 - k, stride, up, dt)
        assert ops.dwconv_bn_train_supported(lo, 1, 1, c, k, stride, up, dt, measured_only=True)
    assert not ops.dwconv_bn_train_routed(2, 7, 7, 8, 5, 1, False, torch.bfloat16)
    assert not ops.dwconv_bn_train_supported(2, 7, 7, 8, 5, 1, False, torch.bfloat16, measured_only=True)


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(1 << 24 | (i + 1) << 16) for i in range(32)]           # distinct, aligned, 64 KiB apart, never dereferenced
    n, h, wd, c, k, dt = 2, 7, 7, 16, 5, 1
    hc, wc = 4, 4
    need = lib.rcx_dwconv_bn_train_workspace_bytes(n, h, wd, c, k, 1, 1, dt)
    assert 0 < need <= 1 << 16
    BAD, UNS, WS = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    off = lambda q, j: ctypes.c_void_p(q.value + j)
    fnames = ("x", "a", "w", "b", "gamma", "beta", "rm", "rv", "y", "u", "mu", "ia", "ws")
    base = dict(zip(fnames, p))

    def fwd(nbytes=need, n=n, h=h, wd=wd, c=c, k=k, stride=1, dt=dt, hc=hc, wc=wc, **kw):
        a = dict(base, **kw)
        return lib.rcx_dwconv_bn_train_fwd(a["x"], a["a"], hc, wc, *[a[j] for j in fnames[2:]], nbytes, n, h, wd, c, k, stride, 0.1, 1e-5, dt, None)

    for j in ("x", "w", "gamma", "beta", "y", "u", "mu", "ia"):
        assert fwd(**{j: None}) == BAD, j
        assert b"null" in lib.rcx_last_error()
    for j in ("rm", "rv"):
        assert fwd(**{j: None}) == BAD, j                                       # a running pointer without its partner
        assert b"together" in lib.rcx_last_error()
    assert fwd(n=0) == BAD and fwd(h=-1) == BAD and fwd(wd=0) == BAD and fwd(c=0) == BAD and fwd(hc=0) == BAD and fwd(wc=-2) == BAD
    assert fwd(n=1, h=1, wd=1) == BAD                                           # R = 1
    assert b"more than one value" in lib.rcx_last_error()
    assert fwd(n=1, h=2, wd=2, stride=2, a=None) == BAD                         # R = 1 at the output of a stride-2 conv
    assert b"more than one value" in lib.rcx_last_error()
    assert fwd(dt=5) == BAD
    assert b"dtype" in lib.rcx_last_error()
    assert fwd(k=4) == UNS and fwd(k=7) == UNS
    assert b"kernel size" in lib.rcx_last_error()
    assert fwd(stride=3, a=None) == UNS and fwd(stride=0, a=None) == UNS
    assert b"stride" in lib.rcx_last_error()
    assert fwd(stride=2) == UNS                                                 # up-add with stride 2
    assert b"stride 1 only" in lib.rcx_last_error()
    for j, v in (("x", off(p[0], 1)), ("y", off(p[8], 1)), ("a", off(p[1], 2)), ("w", off(p[2], 2)), ("b", off(p[3], 1)), ("rm", off(p[6], 2)), ("u", off(p[9], 2)),
                 ("ia", off(p[11], 3)), ("ws", off(p[12], 2))):
        assert fwd(**{j: v}) == BAD, j
        assert b"aligned" in lib.rcx_last_error()
    xb, ub = 2 * n * h * wd * c, 4 * n * h * wd * c
    for j, v in (("y", base["x"]), ("y", off(base["x"], xb - 2)), ("u", base["a"]), ("u", off(base["a"], 4 * n * hc * wc * c - 4)), ("mu", base["w"]),
                 ("mu", off(base["w"], 100 * c - 4)), ("ia", base["mu"]), ("rm", base["b"]), ("rv", base["rm"]), ("ws", base["x"]), ("ws", off(base["y"], 64)),
                 ("ia", off(base["ws"], need - 4)), ("mu", off(base["u"], ub - 4)), ("y", off(base["u"], 8))):
        assert fwd(**{j: v}) == BAD, (j, v)                                     # an output or the workspace overlaps an input or another output
        assert b"alias" in lib.rcx_last_error()
    assert fwd(n=1, h=1 << 15, wd=1 << 15, c=2, k=3, a=None) == UNS             # 2^31 elements
    assert b"2^31" in lib.rcx_last_error()
    assert fwd(nbytes=need - 1) == WS and fwd(ws=None, nbytes=0) == WS
    assert b"workspace" in lib.rcx_last_error()
    assert fwd(a=None, b=None, rm=None, rv=None, nbytes=need - 1) == WS         # every optional input NULL: the call gets as far as the workspace

    bnames = ("x", "a", "u", "g", "w", "gamma", "mu", "ia", "gx", "ga", "gw", "gb", "gga", "gbe", "ws")
    bbase = dict(zip(bnames, p))
    outs = bnames[8:14]

    def bwd(nbytes=need, n=n, h=h, wd=wd, c=c, k=k, stride=1, dt=dt, hc=hc, wc=wc, **kw):
        a = dict(bbase, **kw)
        return lib.rcx_dwconv_bn_train_bwd(a["x"], a["a"], hc, wc, *[a[j] for j in bnames[2:]], nbytes, n, h, wd, c, k, stride, dt, None)

    for j in ("x", "u", "g", "w", "gamma", "mu", "ia"):
        assert bwd(**{j: None}) == BAD, j
        assert b"null" in lib.rcx_last_error()
    assert bwd(**{j: None for j in outs}) == BAD
    assert b"every output" in lib.rcx_last_error()
    assert bwd(a=None) == BAD                                                   # ga asked for in the plain form
    assert b"ga without a" in lib.rcx_last_error()
    assert bwd(n=0) == BAD and bwd(c=-3) == BAD and bwd(dt=3) == BAD and bwd(n=1, h=1, wd=1) == BAD and bwd(hc=0) == BAD
    assert bwd(k=4) == UNS and bwd(stride=3, a=None, ga=None) == UNS and bwd(stride=2) == UNS
    assert bwd(x=off(p[0], 1)) == BAD and bwd(g=off(p[3], 1)) == BAD and bwd(gx=off(p[8], 1)) == BAD and bwd(u=off(p[2], 2)) == BAD
    assert bwd(ga=off(p[9], 2)) == BAD and bwd(gw=off(p[10], 1)) == BAD and bwd(ws=off(p[14], 1)) == BAD
    assert b"aligned" in lib.rcx_last_error()
    for j, v in (("gx", bbase["x"]), ("gx", bbase["g"]), ("ga", bbase["a"]), ("gw", bbase["w"]), ("gb", bbase["mu"]), ("gbe", bbase["gga"]), ("ws", bbase["ia"]),
                 ("ws", bbase["gx"]), ("gx", off(bbase["ws"], 8)), ("gb", off(bbase["gw"], 100 * c - 4)), ("ga", off(bbase["u"], 16))):
        assert bwd(**{j: v}) == BAD, j
        assert b"alias" in lib.rcx_last_error()
    assert bwd(n=1, h=1 << 15, wd=1 << 15, c=2, k=3, a=None, ga=None) == UNS
    assert bwd(nbytes=need - 1) == WS and bwd(ws=None, nbytes=0) == WS
    for keep in outs:                                                           # each output alone is a valid request (ga needs a, which is given)
        assert bwd(nbytes=need - 1, **{j: None for j in outs if j != keep}) == WS, keep
    assert bwd(a=None, ga=None, nbytes=need - 1) == WS


def test_functions_refuse_bad_arguments_and_cpu_tensors():
    d = conv64.case((2, 8, 1, 1), torch.float32, "normal", (5, 1, True))
    x = d["x"].expand(2, 8, 3, 3).contiguous(memory_format=torch.channels_last)
    par = [d[j] for j in ("w", "b", "gamma", "beta")]
    with pytest.raises(_lib.RcxError):
        ops.dwconv_bn_train(x, *par)
    with pytest.raises(ValueError):
        ops.dwconv_bn_train(x[0], *par)
    with pytest.raises(ValueError):
        ops.dwconv_bn_train(x.double(), *par)
    with pytest.raises(ValueError):
        ops.dwconv_bn_train_backward(x[0], x, d["w"], d["gamma"], torch.zeros(2, 8), x)
    with pytest.raises(_lib.RcxError):
        ops.DwConvBnFn.apply(x.requires_grad_(True), None, *par, None, None, 1, 0.1, 1e-5)


# ---- the router ---------------------------------------------------------------------------------------------------------------------------------------------

def _hosts(net):
    out = []
    for m in net.modules():
        if isinstance(m, recattn.RecAttn2d):
            out += [m.down[0], m.conv]
        elif isinstance(m, (recattn.LinearAttention, lsmodels.LinearAttention3)):
            out.append(m.pe)
    return out


def test_router_marks_the_slice_mixers_of_recnext_t_and_keeps_the_model():
    torch.manual_seed(1)
    net = lsmodels.create_model("recnext_t", num_classes=10)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    params = {k: id(p) for k, p in net.named_parameters()}
    buffers = {k: id(b) for k, b in net.named_buffers()}
    mods = {k: (id(m), type(m)) for k, m in net.named_modules()}
    ra = sum(isinstance(m, recattn.RecAttn2d) for m in net.modules())
    la3 = sum(isinstance(m, lsmodels.LinearAttention3) for m in net.modules())
    hosts = _hosts(net)
    assert ra and la3 and len(hosts) == 3 * ra + la3                            # three a RecAttn2d block, one a LinearAttention3 block
    assert not any("_fused_conv_norm_train" in m.__dict__ for m in net.modules())          # nothing is marked unless asked for
    assert models.use_fused_conv_norm_train(net) == 3 * ra + la3
    assert models.use_fused_conv_norm_train(net) == 0 and models.use_fused_conv_norm_train(net, all_shapes=True) == 0        # idempotent
    assert all(m.__dict__["_fused_conv_norm_train"] == "all" for m in hosts)
    marked = [m for m in net.modules() if "_fused_conv_norm_train" in m.__dict__]
    assert {id(m) for m in marked} == {id(m) for m in hosts}                    # those modules and no others
    assert not any("_fused_conv_norm_train" in m.lk.__dict__ for m in net.modules() if isinstance(m, lsmodels.RepVGGDW))    # RepVGGDW has its own operator
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert {k: id(p) for k, p in net.named_parameters()} == params and {k: id(b) for k, b in net.named_buffers()} == buffers
    assert {k: (id(m), type(m)) for k, m in net.named_modules()} == mods
    fresh = lsmodels.create_model("recnext_t", num_classes=10)
    fresh.load_state_dict(net.state_dict(), strict=True)
    net.load_state_dict(fresh.state_dict(), strict=True)
    assert all(m.__dict__["_fused_conv_norm_train"] == "all" for m in _hosts(copy.deepcopy(net)))
    a_net = models.create_model("recnext_a0", num_classes=10)                   # the A family: three a RecAttn2d, no conv bias
    ra_a = sum(isinstance(m, recattn.RecAttn2d) for m in a_net.modules())
    assert ra_a and models.use_fused_conv_norm_train(a_net) == 3 * ra_a
    assert models.use_fused_conv_norm_train(_builders()["models"]()) == 0       # a model without slice mixers


def test_routed_tiny_model_equals_the_unrouted_one_on_the_cpu():
    torch.manual_seed(2)
    ref = _builders()["lsmodels"]()
    hip = copy.deepcopy(ref)
    models.use_fused_conv_norm_train(hip, all_shapes=True)
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

def aten_chain(d, form, bias):
    """The unfused ConvNorm on ATen in float32 with autograd: -> (outputs by conv64's names, the float32 (2, C) statistics the chain itself formed)."""
    k, stride, up = form
    c = d["x"].shape[1]
    x = d["x"].clone().requires_grad_(True)
    a = d["a"].clone().requires_grad_(True) if up else None
    names = ("w", "b", "gamma", "beta") if bias else ("w", "gamma", "beta")
    p = {j: d[j].clone().requires_grad_(True) for j in names}
    run = {j: d[j].clone() for j in ("running_mean", "running_var")}
    z = x + F.interpolate(a, size=x.shape[2:], mode="nearest") if up else x
    u = F.conv2d(z, p["w"], p.get("b"), stride=stride, padding=k // 2, groups=c)
    y = F.batch_norm(u, run["running_mean"], run["running_var"], p["gamma"], p["beta"], True, conv64.MOM, conv64.EPS)
    leaves = [x] + ([a] if up else []) + [p[j] for j in names]
    grads = list(torch.autograd.grad(y, leaves, d["g"]))
    out = dict(run, y=y.detach(), u=u.detach(), gx=grads.pop(0))
    if up:
        out["ga"] = grads.pop(0)
    out.update({"g" + j: t for j, t in zip(names, grads)})
    with torch.no_grad():
        _, mean_u, invstd_u = torch.native_batch_norm(u, None, None, None, None, True, 0.0, conv64.EPS)
    out.update(mean_u=mean_u, invstd_u=invstd_u)
    return out, torch.stack([mean_u, invstd_u])


@pytest.mark.parametrize("dist", bn64.DISTS)
@pytest.mark.parametrize("form", conv64.FORMS, ids=_FORM_IDS)
@pytest.mark.parametrize("shape", conv64.SHAPES + [bn64.UNALIGNED], ids=lambda s: "x".join(map(str, s)))
def test_reference_bounds_hold_for_the_aten_chain(shape, form, dist, record_property):
    d = conv64.case(shape, torch.float32, dist, form)
    f32 = torch.float32
    worst = {}
    for bias in (True, False):
        got, stats = aten_chain(d, form, bias)
        tag = f"{shape} {form} {dist} bias={bias} "
        ref = conv64.forward_ref(d, form, bias=bias)
        for name in ("y", "u", "mean_u", "invstd_u", "running_mean", "running_var"):
            worst[name] = max(worst.get(name, 0.0), conv64.check(got[name], ref[name], f32, tag + name))
        refb = conv64.backward_ref(d, form, stats, bias=bias)
        for name in ("gx", "gw", "ggamma", "gbeta") + (("ga",) if form[2] else ()) + (("gb",) if bias else ()):
            worst[name] = max(worst.get(name, 0.0), conv64.check(got[name], refb[name], f32, tag + name))
    record_property("worst_ratio", {j: round(v, 3) for j, v in worst.items()})
    print(f"  {shape} {form} {dist}: " + ", ".join(f"{j} {v:.2f}" for j, v in worst.items()))
    assert max(worst.values()) <= 24.0
