"""CPU: the channel mixers' BatchNorm + GELU and BatchNorm + residual without a GPU (rcx_bn_act_*, recnext_amd/bnact.py,
models.use_fused_mixer_norms_train): the declarations, the refusals that come before any HIP call, the routing table, the router, and the float64
references and bounds of tests/act64.py held against ATen's float32 ``gelu(native_batch_norm(x))`` / ``r + s * native_batch_norm(x)`` and their autograd
on the CPU, which shows the bounds are held by something other than the code under test."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from recnext_amd import _lib, bnact, lsmodels, models, ops
from tests import act64, bn64
from tests.util import GOLDEN

ROOT = os.path.join(os.path.dirname(GOLDEN), "..")
ENTRIES = ("rcx_bn_act_supported", "rcx_bn_act_workspace_bytes", "rcx_bn_act_train_fwd", "rcx_bn_act_train_bwd")
GELU, ADD = 0, 1


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
    assert "#define RCX_BN_EPI_GELU 0" in header and "#define RCX_BN_EPI_ADD 1" in header and bnact.EPILOGUES == {"gelu": 0, "add": 1}
    doc = header[header.index("The two BatchNorms of a channel mixer"):header.index("int rcx_bn_act_supported(")]
    for cite in ("lsnet/model/recattn.py:199-205", ":240-251", ":254-263", ":208-223", "model/recnext.py:125-131", "engine.py:38-71"):
        assert cite in doc, cite
    for f in ("bn_act_supported", "bn_act_routed", "bn_gelu_train", "bn_gelu_train_backward", "bn_add_train", "bn_add_train_backward", "BnGeluFn", "BnAddFn"):
        assert getattr(ops, f) is getattr(bnact, f) and getattr(ops, f).__module__ == "recnext_amd.bnact", f
    makefile = open(os.path.join(ROOT, "recnext_amd", "csrc", "Makefile")).read()
    tus = [l for l in makefile.splitlines() if l.startswith("SCRATCH_TUS")][0]
    assert "rcx_bnact" in tus.split()
    assert "k_bnact_" in open(os.path.join(ROOT, "tools", "check_scratch.py")).read()


def test_supported_and_workspace_queries(lib):
    sup, q = lib.rcx_bn_act_supported, lib.rcx_bn_act_workspace_bytes
    for n, c, h, w in bn64.SHAPES + [bn64.UNALIGNED]:
        for dt in (0, 1, 2):
            for rdt, epi in ((dt, GELU), (dt, ADD), (0, ADD)):
                assert sup(n, h, w, c, dt, rdt, epi) == 1
                assert q(n, h, w, c, dt, rdt, epi) == lib.rcx_batchnorm_workspace_bytes(n, h, w, c, dt) > 0        # the BatchNorm's own scheme
    for bad in ((0, 7, 7, 8, 1, 1, GELU), (2, 7, 7, 0, 1, 1, ADD), (2, 7, 7, 8, 3, 3, GELU), (2, 7, 7, 8, 1, 1, 2), (2, 7, 7, 8, 1, 1, -1),
                (2, 7, 7, 8, 1, 0, GELU), (2, 7, 7, 8, 1, 2, ADD), (2, 7, 7, 8, 0, 1, ADD)):
        assert sup(*bad) == 0 and q(*bad) == 0, bad
    assert sup(1, 1 << 15, 1 << 15, 1, 1, 1, GELU) == 1 and sup(1, 1 << 15, 1 << 15, 2, 1, 1, GELU) == 0          # 2^30 elements, 2^31 elements
    bf = torch.bfloat16
    assert ops.bn_act_supported(2, 7, 7, 8, bf, "gelu") and ops.bn_act_supported(2, 7, 7, 8, bf, "add", rdtype=torch.float32)
    assert not ops.bn_act_supported(2, 7, 7, 8, torch.float64, "gelu") and not ops.bn_act_supported(2, 7, 7, 8, bf, "relu")
    assert not ops.bn_act_supported(2, 7, 7, 8, bf, "gelu", rdtype=torch.float32) and not ops.bn_act_supported(2, 7, 7, 8, bf, "add", rdtype=torch.float16)


def test_routing_table_is_keyed_by_channels_element_size_and_epilogue():
    """(C, element size of u, epilogue) -> (lo, hi) rows, as batchnorm.ROUTED plus the epilogue; a rule on (R = N H W, C, element size, epilogue) alone."""
    for key, (lo, hi) in bnact.ROUTED.items():
        c, es, epi = key
        assert isinstance(c, int) and c > 0 and es in (2, 4) and epi in bnact.EPILOGUES and isinstance(lo, int) and isinstance(hi, int) and 0 < lo <= hi, key
        dt = torch.float32 if es == 4 else torch.bfloat16
        assert ops.bn_act_routed(1, 1, lo, c, dt, epi) and ops.bn_act_routed(hi, 1, 1, c, dt, epi) and ops.bn_act_supported(1, lo, 1, c, dt, epi, measured_only=True)
        assert not ops.bn_act_routed(1, 1, lo - 1, c, dt, epi) and not ops.bn_act_routed(1, hi + 1, 1, c, dt, epi)
        if es == 2:
            assert ops.bn_act_routed(1, 1, lo, c, torch.float16, epi)                      # the element size, not the type
    assert not ops.bn_act_routed(128, 14, 14, 7, torch.bfloat16, "gelu") and not ops.bn_act_routed(128, 14, 14, 7, torch.float32, "add")
    assert not ops.bn_act_supported(128, 14, 14, 7, torch.bfloat16, "gelu", measured_only=True) and ops.bn_act_supported(128, 14, 14, 7, torch.bfloat16, "gelu")


def test_argument_errors_without_a_gpu(lib):
    p = [ctypes.c_void_p(1 << 20 | (i + 1) << 14) for i in range(12)]         # distinct, aligned, 16 KiB apart, never dereferenced
    u, r, sc, out, w, b, rm, rv, sm, si, ws, g = p
    n, h, wd, c, dt = 2, 7, 7, 16, 1
    need = lib.rcx_bn_act_workspace_bytes(n, h, wd, c, dt, dt, GELU)
    assert 0 < need <= 1 << 14
    BAD, UNS, WS = _lib.ERR_BAD_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_WORKSPACE
    off = lambda q, k: ctypes.c_void_p(q.value + k)

    def fwd(u=u, r=r, sc=sc, out=out, w=w, b=b, rm=rm, rv=rv, sm=sm, si=si, ws=ws, nbytes=need, n=n, h=h, wd=wd, c=c, epi=ADD, dt=dt, rdt=dt):
        return lib.rcx_bn_act_train_fwd(u, r, sc, out, w, b, rm, rv, sm, si, ws, nbytes, n, h, wd, c, 0.1, 1e-5, epi, dt, rdt, None)

    for epi in (GELU, ADD):
        for k in ("u", "out", "w", "b", "sm", "si"):
            assert fwd(epi=epi, **{k: None}) == BAD, (epi, k)
            assert b"null" in lib.rcx_last_error()
        assert fwd(epi=epi, rm=None) == BAD and fwd(epi=epi, rv=None) == BAD      # one running pointer without the other
        assert fwd(epi=epi, n=0) == BAD and fwd(epi=epi, h=-1) == BAD and fwd(epi=epi, c=0) == BAD and fwd(epi=epi, dt=5, rdt=5) == BAD
        assert fwd(epi=epi, n=1, h=1, wd=1) == BAD                                # R = 1 with batch statistics
        assert b"more than one value" in lib.rcx_last_error()
        for k, v in (("u", off(u, 1)), ("out", off(out, 1)), ("w", off(w, 2)), ("sm", off(sm, 2)), ("ws", off(ws, 2))):
            assert fwd(epi=epi, **{k: v}) == BAD, (epi, k)
            assert b"aligned" in lib.rcx_last_error()
        for k, v in (("out", u), ("out", off(u, 2 * (n * h * wd * c - 1))), ("sm", w), ("si", sm), ("rm", b), ("ws", u), ("si", off(ws, need - 4))):
            assert fwd(epi=epi, **{k: v}) == BAD, (epi, k)                        # an output or the workspace overlaps an input or another output
            assert b"alias" in lib.rcx_last_error()
        assert fwd(epi=epi, n=1, h=1 << 15, wd=1 << 15, c=2) == UNS               # 2^31 elements
        assert fwd(epi=epi, nbytes=need - 1) == WS and fwd(epi=epi, ws=None, nbytes=0) == WS
    assert fwd(epi=2) == BAD and fwd(epi=-1) == BAD
    assert b"epilogue" in lib.rcx_last_error()
    assert fwd(epi=ADD, r=None) == BAD and fwd(epi=GELU, r=None, sc=None, nbytes=need - 1) == WS    # r is ADD's; the GELU takes none (every call here is refused)
    assert fwd(epi=ADD, sc=None, nbytes=need - 1) == WS                            # scale may be NULL
    assert fwd(epi=ADD, out=r) == BAD and fwd(epi=ADD, out=off(r, 2 * (n * h * wd * c - 1))) == BAD    # r may not overlap out
    assert b"alias" in lib.rcx_last_error()
    assert fwd(epi=GELU, out=r, nbytes=need - 1) == WS                            # ... which the GELU does not read
    assert fwd(epi=ADD, r=off(r, 1)) == BAD and fwd(epi=ADD, sc=off(sc, 2)) == BAD and fwd(epi=ADD, rdt=0, r=off(r, 2)) == BAD
    assert fwd(epi=ADD, rdt=0, out=off(r, 4 * (n * h * wd * c - 1))) == BAD       # a float32 residual is twice as long
    assert fwd(epi=ADD, rdt=2) == UNS and fwd(epi=GELU, rdt=0) == UNS and fwd(epi=ADD, rdt=7) == BAD
    assert fwd(epi=ADD, rdt=0, nbytes=need - 1) == WS

    def bwd(u=u, g=g, sc=sc, w=w, b=b, mean=sm, invstd=si, gu=out, gw=rm, gb=rv, ws=ws, nbytes=need, n=n, h=h, wd=wd, c=c, epi=GELU, dt=dt, rdt=dt):
        return lib.rcx_bn_act_train_bwd(u, g, sc, w, b, mean, invstd, gu, gw, gb, ws, nbytes, n, h, wd, c, epi, dt, rdt, None)

    for epi in (GELU, ADD):
        for k in ("u", "g", "w", "mean", "invstd"):
            assert bwd(epi=epi, **{k: None}) == BAD, (epi, k)
        assert bwd(epi=epi, gu=None, gw=None, gb=None) == BAD
        assert b"every output" in lib.rcx_last_error()
        assert bwd(epi=epi, gw=None) == BAD and bwd(epi=epi, gb=None) == BAD      # the pair comes together
        assert bwd(epi=epi, n=0) == BAD and bwd(epi=epi, dt=3, rdt=3) == BAD and bwd(epi=epi, n=1, h=1, wd=1) == BAD
        assert bwd(epi=epi, g=off(g, 1)) == BAD and bwd(epi=epi, gu=off(out, 1)) == BAD and bwd(epi=epi, gw=off(rm, 2)) == BAD and bwd(epi=epi, ws=off(ws, 1)) == BAD
        for k, v in (("gu", u), ("gu", g), ("gw", w), ("gb", sm), ("gb", rm), ("ws", si), ("ws", out), ("gu", off(ws, 8))):
            assert bwd(epi=epi, **{k: v}) == BAD, (epi, k)
            assert b"alias" in lib.rcx_last_error()
        assert bwd(epi=epi, n=1, h=1 << 15, wd=1 << 15, c=2) == UNS
        assert bwd(epi=epi, nbytes=need - 1) == WS and bwd(epi=epi, ws=None, nbytes=0) == WS
        assert bwd(epi=epi, gu=None, nbytes=need - 1) == WS and bwd(epi=epi, gw=None, gb=None, nbytes=need - 1) == WS
    assert bwd(epi=3) == BAD and bwd(epi=GELU, b=None) == BAD and bwd(epi=ADD, b=None, sc=None, nbytes=need - 1) == WS
    assert bwd(epi=GELU, rdt=0) == UNS and bwd(epi=ADD, rdt=0, nbytes=need - 1) == WS and bwd(epi=ADD, rdt=0, g=off(g, 2)) == BAD


def test_functions_refuse_bad_arguments_and_cpu_tensors():
    x = torch.randn(2, 8, 3, 3).contiguous(memory_format=torch.channels_last)
    w, b = torch.ones(8), torch.zeros(8)
    for call in (lambda: ops.bn_gelu_train(x, w, b), lambda: ops.bn_add_train(x, x, w, b), lambda: ops.bn_gelu_train_backward(x, x, w, b, b, w),
                 lambda: ops.bn_add_train_backward(x, x, w, b, w), lambda: ops.BnGeluFn.apply(x.clone().requires_grad_(True), w, b, None, None, 0.1, 1e-5),
                 lambda: ops.BnAddFn.apply(x.clone().requires_grad_(True), x, None, w, b, None, None, 0.1, 1e-5)):
        with pytest.raises(_lib.RcxError):
            call()
    with pytest.raises(ValueError):
        ops.bn_gelu_train(x[0], w, b)
    with pytest.raises(ValueError):
        ops.bn_gelu_train(x.double(), w, b)
    with pytest.raises(ValueError):
        ops.bn_add_train(x[0], x, w, b)


# ---- the router ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["recnext_m1", "recnext_t", "recnext_t_share_channel"])
def test_router_marks_every_mixer_and_stem_and_keeps_keys_and_tensors(name):
    torch.manual_seed(1)
    net = models.create_model(name)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    params = {k: id(p) for k, p in net.named_parameters()}
    buffers = {k: id(b) for k, b in net.named_buffers()}
    mods = {k: id(m) for k, m in net.named_modules()}
    hosts = (models.MetaNeXtBlock, models.Downsample, lsmodels.MetaNeXtBlock, lsmodels.Downsample)
    mixers = [m.channel_mixer for m in net.modules() if isinstance(m, hosts)]
    stems = [m for m in net.modules() if isinstance(m, (models.RecNextStem, lsmodels.RecNextStem))]
    depth = {"recnext_m1": 23, "recnext_t": 20, "recnext_t_share_channel": 20}[name]
    assert len(mixers) == depth + 3 and len(stems) == 1                         # every block, the three Downsamples, the stem
    assert models.use_fused_mixer_norms_train(net, all_shapes=(name == "recnext_t")) == depth + 4
    assert models.use_fused_mixer_norms_train(net) == 0                         # idempotent
    for host in mixers + stems:
        mark = host.__dict__[bnact.ATTR]
        layers = list(host if isinstance(host, nn.Sequential) else host.stem)
        assert mark[0] == "measured" and len(mark) == 1 + len(layers) and all(a is b for a, b in zip(mark[1:], layers))
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert {k: id(p) for k, p in net.named_parameters()} == params and {k: id(b) for k, b in net.named_buffers()} == buffers
    assert {k: id(m) for k, m in net.named_modules()} == mods
    fresh = models.create_model(name)
    fresh.load_state_dict(net.state_dict(), strict=True)
    net.load_state_dict(fresh.state_dict(), strict=True)
    twin = copy.deepcopy(net)                                                   # a copy is marked with its own layers
    for m in twin.modules():
        if isinstance(m, hosts):
            assert all(a is b for a, b in zip(m.channel_mixer.__dict__[bnact.ATTR][1:], m.channel_mixer))


def test_marked_tiny_model_equals_the_unmarked_one_on_the_cpu():
    torch.manual_seed(2)
    ref = models.RecNext(family="m", embed_dim=(8, 16, 32, 64), depth=(1, 1, 1, 1), num_classes=10, drop_path=0.5,
                         token_mixer=lambda dim, stage: nn.Conv2d(dim, dim, 3, padding=1, groups=dim))
    hip = copy.deepcopy(ref)
    assert models.use_fused_mixer_norms_train(hip, all_shapes=True) == 4 + 3 + 1
    x, y = torch.randn(2, 3, 64, 64), torch.tensor([1, 7])
    for net in (ref, hip):
        net.train()
        torch.manual_seed(5)                                                    # the DropPath masks
        F.cross_entropy(net(x), y).backward()
    for (k, p), (_, q) in zip(ref.named_parameters(), hip.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
    for (k, a), (_, b) in zip(ref.named_buffers(), hip.named_buffers()):
        assert torch.equal(a, b), k
    ref.eval(), hip.eval()
    with torch.no_grad():
        assert torch.equal(ref(x), hip(x))


# ---- the references and their bounds, against ATen's float32 chain -------------------------------------------------------------------------------------------

_ATEN = [(dt, dist) for dt in (torch.float32, torch.bfloat16) for dist in bn64.dists_of(dt)]


@pytest.mark.parametrize("dt,dist", _ATEN, ids=[f"{'f32' if dt == torch.float32 else 'bf16'}-{dist}" for dt, dist in _ATEN])
def test_reference_bounds_hold_for_aten_float32(dt, dist, record_property):
    """ATen's float32 chain on float32 and on bf16-valued inputs stays inside the 24 units for every output of both epilogues, over bn64's shapes."""
    worst = {}
    for shape in bn64.SHAPES:
        for k, v in _aten_case(shape, dt, dist).items():
            worst[k] = max(worst.get(k, 0.0), v)
    record_property("worst_ratio", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 24.0


def _aten_case(shape, dt, dist):
    d, e = bn64.case(shape, dt, dist), act64.extra(shape, dt, dist)
    f32 = torch.float32
    worst = {}

    def leaves():
        return d["x"].clone().requires_grad_(True), d["weight"].clone().requires_grad_(True), d["bias"].clone().requires_grad_(True)

    x, w, b = leaves()
    rm, rv = d["running_mean"].clone(), d["running_var"].clone()
    y, mean, invstd = torch.native_batch_norm(x, w, b, rm, rv, True, bn64.MOMENTUM, bn64.EPS)
    z = F.gelu(y)
    ref = act64.gelu_forward_ref(d["x"], d["weight"], d["bias"], bn64.EPS, running_mean=d["running_mean"], running_var=d["running_var"])
    for name, got in (("z", z), ("save_mean", mean), ("save_invstd", invstd), ("running_mean", rm), ("running_var", rv)):
        worst[name] = bn64.check(got.detach(), ref[name], f32, name)
    grads = torch.autograd.grad(z, (x, w, b), d["gy"])
    refb = act64.gelu_backward_ref(d["x"], d["gy"], d["weight"], d["bias"], mean.detach(), invstd.detach())
    for name, got in zip(("gx", "gweight", "gbias"), grads):
        worst[name] = bn64.check(got, refb[name], f32, "gelu " + name)

    for tag, scale in (("", None), ("_scaled", e["scale"])):
        x, w, b = leaves()
        r = e["r"].clone().requires_grad_(True)
        y, mean, invstd = torch.native_batch_norm(x, w, b, None, None, True, bn64.MOMENTUM, bn64.EPS)
        out = r + (y if scale is None else y * scale.view(-1, 1, 1, 1))
        ref = act64.add_forward_ref(d["x"], e["r"], scale, d["weight"], d["bias"], bn64.EPS)
        worst["out" + tag] = bn64.check(out.detach(), ref["out"], f32, "out" + tag)
        gx, gw, gb, gr = torch.autograd.grad(out, (x, w, b, r), d["gy"])
        refb = act64.add_backward_ref(d["x"], d["gy"], scale, d["weight"], mean.detach(), invstd.detach())
        for name, got in (("gx", gx), ("gweight", gw), ("gbias", gb)):
            worst["add_" + name + tag] = bn64.check(got, refb[name], f32, "add " + name + tag)
        assert torch.equal(gr, d["gy"])
    return worst
