"""GPU: the channel mixers' BatchNorm + GELU and BatchNorm + residual (rcx_bn_act_*, ops.bn_gelu_train / bn_add_train and their backwards, ops.BnGeluFn /
BnAddFn, models.use_fused_mixer_norms_train).

1  every output of both epilogues, element by element, against the float64 references of tests/act64.py under their bounds (K = 24 units of u32, never
   raised): bn64's nine shapes and a tensor whose pointer is only element-aligned, float32 / bf16 / f16, bn64's input distributions, with and without
   running buffers (one test item per dtype and distribution, walking the shapes), ADD without a scale and with one holding an exact 0 and 1 / keep, a float32 residual beside a 16-bit u, every NULL combination of
   the backward's outputs; each case's worst ratio is recorded.  One GELU case spans pre-activations of +-12;
2  repeat launches bit for bit and tests/guard.py's properties A - D; the Functions under autograd against the direct calls; what BnGeluFn saves; R = 1;
3  a routed T-style block, M block, Downsample, stem and a block with DropPath against unrouted deep copies; every fallback condition keeps the chain bit
   for bit; one training step of a T-style model, alone and together with the other opt-in training operators."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from recnext_amd import _lib, batchnorm, bnact, layers, lsmodels, models, ops
from tests import act64, bn64, guard

DEV = torch.device("cuda:0")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
GUARDED = tuple(guard.LIBRARY_MODULES) + ("recnext_amd.batchnorm", "recnext_amd.bnact")
_DT_IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
# every dtype x every distribution the dtype can hold (2 + 1e-3 N(0, 1) is float32 only); a case walks every shape and the unaligned tensor
CASES = [(dt, dist) for dt in DTYPES for dist in bn64.dists_of(dt)]
SHAPES = [(s, False) for s in bn64.SHAPES] + [(bn64.UNALIGNED, True)]
f32 = torch.float32
HYPER = (bn64.MOMENTUM, bn64.EPS)


def cl(t, dt, unaligned=False):
    """NCHW CPU float32 -> dense channels_last on the GPU in dt; unaligned: its first element one element past a 16-byte boundary."""
    n, c, h, w = t.shape
    if not unaligned:
        return t.to(DEV).contiguous(memory_format=torch.channels_last).to(dt)
    buf = torch.empty(t.numel() + 1, dtype=dt, device=DEV)
    v = buf[1:].view(n, h, w, c).permute(0, 3, 1, 2)
    v.copy_(t.to(DEV))
    assert v.data_ptr() % 16 == buf.element_size() and batchnorm._dense_nhwc(v)
    return v


def _gpu(d, *names):
    return [d[k].to(DEV) for k in names]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,dist", CASES, ids=[f"{_DT_IDS[dt]}-{dist}" for dt, dist in CASES])
def test_every_output_against_float64(dt, dist, record_property):
    worst = {}
    for shape, unaligned in SHAPES:
        for k, v in _every_output(shape, unaligned, dt, dist).items():
            worst[k] = max(worst.get(k, 0.0), v)
    record_property("worst_ratio", {k: round(v, 3) for k, v in worst.items()})
    print(f"  {dt} {dist}: worst err / u32 bound units over the shapes: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def _every_output(shape, unaligned, dt, dist):
    """One shape of test_every_output_against_float64: -> the worst ratio per output."""
    d, e = bn64.case(shape, dt, dist), act64.extra(shape, dt, dist)
    n, c, h, w = shape
    u, g = cl(d["x"], dt, unaligned), cl(d["gy"], dt, unaligned)
    weight, bias = _gpu(d, "weight", "bias")
    tag = f"{shape} {dt} {dist} "
    worst = {}

    def hold(name, got, pair, odt):
        worst[name] = max(worst.get(name, 0.0), bn64.check(got, pair, odt, tag + name))

    # ---- GELU: with and without running buffers, then its backward from the kernel's own saved statistics
    rm, rv = _gpu(d, "running_mean", "running_var")
    z, mean, invstd = ops.bn_gelu_train(u, weight, bias, rm, rv, *HYPER)
    assert z.dtype == dt and z.shape == u.shape and batchnorm._dense_nhwc(z) and mean.dtype == invstd.dtype == f32 and mean.shape == invstd.shape == (c,)
    ref = act64.gelu_forward_ref(d["x"], d["weight"], d["bias"], bn64.EPS, running_mean=d["running_mean"], running_var=d["running_var"])
    for name, got, odt in (("z", z, dt), ("save_mean", mean, f32), ("save_invstd", invstd, f32), ("running_mean", rm, f32), ("running_var", rv, f32)):
        hold(name, got, ref[name], odt)
    z2, mean2, invstd2 = ops.bn_gelu_train(u, weight, bias, None, None, *HYPER)
    assert torch.equal(z2, z) and torch.equal(mean2, mean) and torch.equal(invstd2, invstd)
    _, bmean, binvstd = ops.batch_norm_train(u, weight, bias, None, None, *HYPER)
    assert torch.equal(bmean, mean) and torch.equal(binvstd, invstd)             # the BatchNorm's own statistics launches
    refb = act64.gelu_backward_ref(d["x"], d["gy"], d["weight"], d["bias"], mean, invstd)
    full = ops.bn_gelu_train_backward(u, g, weight, bias, mean, invstd)
    assert full[0].dtype == dt and batchnorm._dense_nhwc(full[0]) and full[1].dtype == full[2].dtype == f32 and full[1].shape == full[2].shape == (c,)
    for name, got, odt in (("gx", full[0], dt), ("gweight", full[1], f32), ("gbias", full[2], f32)):
        hold("gelu_" + name, got, refb[name], odt)
    for need_x, need_p in ((True, False), (False, True)):
        part = ops.bn_gelu_train_backward(u, g, weight, bias, mean, invstd, need_input_grad=need_x, need_param_grads=need_p)
        assert (part[0] is None) == (not need_x) and (part[1] is None) == (part[2] is None) == (not need_p)
        assert all(got is None or torch.equal(got, want) for got, want in zip(part, full)), (need_x, need_p)
    with pytest.raises(ValueError):
        ops.bn_gelu_train_backward(u, g, weight, bias, mean, invstd, need_input_grad=False, need_param_grads=False)

    # ---- ADD: no scale, a scale holding an exact 0 and 1 / keep; a residual of u's type and, beside a 16-bit u, a float32 one
    scale = e["scale"].to(DEV)
    forms = [(dt, None), (dt, scale)] + ([(f32, scale)] if dt != f32 else [])
    for i, (rdt, sc) in enumerate(forms):
        sfx = ("_r32" if rdt != dt else "") + ("_scaled" if sc is not None else "")
        r, gr = cl(e["r"], rdt, unaligned), cl(d["gy"], rdt, unaligned)
        rm, rv = _gpu(d, "running_mean", "running_var")
        out, amean, ainvstd = ops.bn_add_train(u, r, weight, bias, sc, rm if i == 0 else None, rv if i == 0 else None, *HYPER)
        assert out.dtype == rdt and out.shape == u.shape and batchnorm._dense_nhwc(out) and torch.equal(amean, mean) and torch.equal(ainvstd, invstd)
        ref = act64.add_forward_ref(d["x"], e["r"], None if sc is None else e["scale"], d["weight"], d["bias"], bn64.EPS,
                                    running_mean=d["running_mean"], running_var=d["running_var"])
        hold("out" + sfx, out, ref["out"], rdt)
        if i == 0:
            hold("running_mean", rm, ref["running_mean"], f32)
            hold("running_var", rv, ref["running_var"], f32)
        if sc is not None:
            assert torch.equal(out[0], r[0])                                     # a dropped sample: exactly the residual
        refb = act64.add_backward_ref(d["x"], d["gy"], None if sc is None else e["scale"], d["weight"], mean, invstd)
        full = ops.bn_add_train_backward(u, gr, weight, mean, invstd, sc)
        assert full[0].dtype == dt and batchnorm._dense_nhwc(full[0]) and full[1].dtype == full[2].dtype == f32
        for name, got, odt in (("gx", full[0], dt), ("gweight", full[1], f32), ("gbias", full[2], f32)):
            hold("add_" + name + sfx, got, refb[name], odt)
        for need_x, need_p in ((True, False), (False, True)):
            part = ops.bn_add_train_backward(u, gr, weight, mean, invstd, sc, need_input_grad=need_x, need_param_grads=need_p)
            assert all(got is None or torch.equal(got, want) for got, want in zip(part, full)) and (part[0] is None) == (not need_x)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=lambda t: _DT_IDS[t])
def test_gelu_saturates_exactly_over_preactivations_of_plus_minus_twelve(dt, record_property):
    """gamma = 7 on inputs spread evenly over +-sqrt 3 standard deviations and beta = 0, +6, -6: y spans +-12 (and -6 .. 18, -18 .. 6).  Past |y| = 6.5,
    1 - |erf(y / sqrt 2)| < 8e-11 < 2^-25: a float32 erf is exactly +-1 there, so z is exactly the rounded y (the HIP BatchNorm's own output: the same
    statistics and the same fma) or exactly 0; the rest stays inside the float64 bound, and gu is finite."""
    n, c, h, w = 4, 24, 8, 8
    gen = torch.Generator().manual_seed(12)
    base = torch.linspace(-1.0, 1.0, n * h * w)
    x = torch.stack([base[torch.randperm(n * h * w, generator=gen)] for _ in range(c)], 1).view(n, h, w, c).permute(0, 3, 1, 2).to(dt).float()
    gz = torch.randn(n, c, h, w, generator=gen).to(dt).float()
    weight = torch.full((c,), 7.0)
    bias = torch.tensor([0.0, 6.0, -6.0]).repeat(c // 3)
    u, g, wg, bg = cl(x, dt), cl(gz, dt), weight.to(DEV), bias.to(DEV)
    z, mean, invstd = ops.bn_gelu_train(u, wg, bg, None, None, *HYPER)
    y, _, _ = ops.batch_norm_train(u, wg, bg, None, None, *HYPER)
    ref = act64.gelu_forward_ref(x, weight, bias, bn64.EPS)
    y64 = bn64.unrows(bn64.forward_ref(x, weight, bias, bn64.EPS)["y"][0], (n, c, h, w)).to(DEV)
    assert float(y64.max()) > 17.5 and float(y64.min()) < -17.5 and float(y64[:, 0].max()) > 11.9 and float(y64[:, 0].min()) < -11.9
    hi, lo = y64 > 6.5, y64 < -6.5
    assert int(hi.sum()) > 100 and int(lo.sum()) > 100
    assert torch.equal(z[hi], y[hi]) and int(torch.count_nonzero(z[lo])) == 0
    worst = bn64.check(z, ref["z"], dt, f"+-12 {dt} z")
    gu, gw, gb = ops.bn_gelu_train_backward(u, g, wg, bg, mean, invstd)
    assert bool(torch.isfinite(gu).all()) and bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all())
    refb = act64.gelu_backward_ref(x, gz, weight, bias, mean, invstd)
    ratios = {"z": worst, "gx": bn64.check(gu, refb["gx"], dt, "+-12 gx"), "gweight": bn64.check(gw, refb["gweight"], f32, "+-12 gweight"),
              "gbias": bn64.check(gb, refb["gbias"], f32, "+-12 gbias")}
    record_property("worst_ratio", {k: round(v, 3) for k, v in ratios.items()})


@pytest.mark.gpu
def test_mixed_alignment_takes_the_element_path_inside_the_bounds(record_property):
    """u aligned to 16 bytes beside an r, g or gz that is only element-aligned, and the reverse: one misaligned pointer among those read V-wide puts the
    whole call on the element path (bn::can_wide); every output stays inside the float64 bounds."""
    shape, dist = bn64.UNALIGNED, "normal"
    worst = {}
    for dt in DTYPES:
        d, e = bn64.case(shape, dt, dist), act64.extra(shape, dt, dist)
        weight, bias = _gpu(d, "weight", "bias")
        scale = e["scale"].to(DEV)
        for rdt in ((dt,) if dt == f32 else (dt, f32)):
            for ua, oa in ((False, True), (True, False)):                       # u unaligned?, the other x-like tensors unaligned?
                u, g, r, gr = cl(d["x"], dt, ua), cl(d["gy"], dt, oa), cl(e["r"], rdt, oa), cl(d["gy"], rdt, oa)
                assert (u.data_ptr() % 16 != 0) == ua and (r.data_ptr() % 16 != 0) == oa and (g.data_ptr() % 16 != 0) == oa
                tag = f"{dt} r {rdt} u unaligned {ua} "
                z, mean, invstd = ops.bn_gelu_train(u, weight, bias, None, None, *HYPER)
                ref = act64.gelu_forward_ref(d["x"], d["weight"], d["bias"], bn64.EPS)
                got = {"z": bn64.check(z, ref["z"], dt, tag + "z")}
                refb = act64.gelu_backward_ref(d["x"], d["gy"], d["weight"], d["bias"], mean, invstd)
                for name, t, odt in zip(("gx", "gweight", "gbias"), ops.bn_gelu_train_backward(u, g, weight, bias, mean, invstd), (dt, f32, f32)):
                    got["gelu_" + name] = bn64.check(t, refb[name], odt, tag + "gelu " + name)
                out, mean, invstd = ops.bn_add_train(u, r, weight, bias, scale, None, None, *HYPER)
                got["out"] = bn64.check(out, act64.add_forward_ref(d["x"], e["r"], e["scale"], d["weight"], d["bias"], bn64.EPS)["out"], rdt, tag + "out")
                refb = act64.add_backward_ref(d["x"], d["gy"], e["scale"], d["weight"], mean, invstd)
                for name, t, odt in zip(("gx", "gweight", "gbias"), ops.bn_add_train_backward(u, gr, weight, mean, invstd, scale), (dt, f32, f32)):
                    got["add_" + name] = bn64.check(t, refb[name], odt, tag + "add " + name)
                for k, v in got.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    record_property("worst_ratio", {k: round(v, 3) for k, v in worst.items()})


def _inputs(shape, dt, seed=5, rdt=None):
    gen = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    u = cl(torch.randn(n, c, h, w, generator=gen) + 0.5, dt)
    g = cl(torch.randn(n, c, h, w, generator=gen), dt)
    r = cl(torch.randn(n, c, h, w, generator=gen), rdt or dt)
    ga = cl(torch.randn(n, c, h, w, generator=gen), rdt or dt)
    vec = lambda s, o: (torch.randn(c, generator=gen) * s + o).to(DEV)
    scale = torch.full((n,), 1.25, device=DEV)
    scale[n // 2] = 0.0
    return u, g, r, ga, scale, vec(0.5, 1.0), vec(0.3, 0.0), vec(0.2, 0.0), (torch.rand(c, generator=gen) + 0.5).to(DEV)


PROP_SHAPES = [(3, 21, 5, 9), (8, 40, 14, 14), (4, 768, 4, 4), (2, 16, 56, 56)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PROP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_repeats_and_guard_bands(shape, dt):
    n, c, h, w = shape
    u, g, r, ga, scale, weight, bias, rmean, rvar = _inputs(shape, dt)
    # A - D, and the repeat launch bit for bit (run_properties asserts it first), without running statistics: they are in-out by contract
    z, mean, invstd = guard.run_properties(lambda uu, ww, bb: ops.bn_gelu_train(uu, ww, bb, None, None, 0.1, 1e-5), (u, weight, bias), modules=GUARDED)
    out, _, _ = guard.run_properties(lambda uu, rr, ss, ww, bb: ops.bn_add_train(uu, rr, ww, bb, ss, None, None, 0.1, 1e-5), (u, r, scale, weight, bias),
                                     modules=GUARDED)
    guard.run_properties(lambda uu, rr, ww, bb: ops.bn_add_train(uu, rr, ww, bb, None, None, None, 0.1, 1e-5), (u, r, weight, bias), modules=GUARDED)
    for need_x, need_p in ((True, True), (True, False), (False, True)):
        guard.run_properties(lambda uu, gg, ww, bb, mm, ii: ops.bn_gelu_train_backward(uu, gg, ww, bb, mm, ii, need_input_grad=need_x, need_param_grads=need_p),
                             (u, g, weight, bias, mean, invstd), modules=GUARDED)
        guard.run_properties(lambda uu, gg, ww, mm, ii, ss: ops.bn_add_train_backward(uu, gg, ww, mm, ii, ss, need_input_grad=need_x, need_param_grads=need_p),
                             (u, ga, weight, mean, invstd, scale), modules=GUARDED)
    if dt != f32:                                                               # the float32 residual beside a 16-bit u
        r32, g32 = r.float(), ga.float()
        guard.run_properties(lambda uu, rr, ss, ww, bb: ops.bn_add_train(uu, rr, ww, bb, ss, None, None, 0.1, 1e-5), (u, r32, scale, weight, bias), modules=GUARDED)
        guard.run_properties(lambda uu, gg, ww, mm, ii, ss: ops.bn_add_train_backward(uu, gg, ww, mm, ii, ss), (u, g32, weight, mean, invstd, scale), modules=GUARDED)
    # the workspace is exactly as large as the query says; outputs, statistics and gradients are this module's own allocations
    need = _lib.load().rcx_bn_act_workspace_bytes(n, h, w, c, ops._DT[dt], ops._DT[dt], 0)
    xb = u.numel() * u.element_size()
    for call, outs in ((lambda: ops.bn_gelu_train(u, weight, bias, None, None, 0.1, 1e-5), [xb, 4 * c, 4 * c]),
                       (lambda: ops.bn_add_train(u, r, weight, bias, scale, None, None, 0.1, 1e-5), [xb, 4 * c, 4 * c]),
                       (lambda: ops.bn_gelu_train_backward(u, g, weight, bias, mean, invstd), [xb, 4 * c, 4 * c]),
                       (lambda: ops.bn_add_train_backward(u, ga, weight, mean, invstd, scale, need_param_grads=False), [xb])):
        with guard.guarded_library(GUARDED) as rec:
            call()
            torch.cuda.synchronize()
            guard.check_guards(rec.arenas)
        ws = [a for a in rec.arenas if a.tensor.dtype == torch.uint8]
        assert [a.nbytes for a in ws] == [need] and need > 0
        assert sorted(a.nbytes for a in rec.arenas if a.tensor.dtype != torch.uint8) == sorted(outs)
    # with running statistics given, only those 2 C floats of the inputs change
    arenas = []
    gu_, gw_, gb_, gm_, gv_ = (guard.guarded_copy(t, 0xFF, arenas) for t in (u, weight, bias, rmean, rvar))
    with guard.guarded_library(GUARDED) as rec:
        got = ops.bn_gelu_train(gu_, gw_, gb_, gm_, gv_, 0.1, 1e-5)
        torch.cuda.synchronize()
        guard.check_guards(rec.arenas + arenas)
    guard.check_inputs_unchanged(arenas[:3])
    for a, old in zip(arenas[3:], (rmean, rvar)):
        changed = (a.buf != a.snapshot).nonzero().flatten()
        assert len(changed) and int(changed.min()) >= guard.GUARD and int(changed.max()) < guard.GUARD + 4 * c
        assert not torch.equal(a.tensor, old) and bool(torch.isfinite(a.tensor).all())
    guard.check_same(got, (z, mean, invstd), "running statistics given against none")

    def both_ways(uu, rr, ss, ww, bb, w2, b2, gg):
        ui = uu.detach().requires_grad_(True)
        leaves = [t.detach().requires_grad_(True) for t in (ww, bb, w2, b2)]
        zz = ops.BnGeluFn.apply(ui, leaves[0], leaves[1], None, None, 0.1, 1e-5)
        oo = ops.BnAddFn.apply(zz, rr, ss, leaves[2], leaves[3], None, None, 0.1, 1e-5)
        return (oo.detach(),) + torch.autograd.grad(oo, [ui] + leaves, gg)
    guard.run_properties(both_ways, (u, r, scale, weight, bias, bias + 1.0, weight - 1.0, ga), modules=GUARDED)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_functions_under_autograd_agree_with_the_direct_calls(dt):
    shape = (5, 16, 13, 11)
    for rdt in ((dt,) if dt == f32 else (dt, f32)):
        u, g, r, ga, scale, weight, bias, rmean, rvar = _inputs(shape, dt, seed=9, rdt=rdt)
        rm, rv = rmean.clone(), rvar.clone()
        z, mean, invstd = ops.bn_gelu_train(u, weight, bias, rm, rv, 0.1, 1e-5)
        want = ops.bn_gelu_train_backward(u, g, weight, bias, mean, invstd)
        for req in ((True, True, True), (True, False, False), (False, True, True), (False, False, True)):
            ui, wi, bi = (t.detach().clone().requires_grad_(q) for t, q in zip((u, weight, bias), req))
            rm2, rv2 = rmean.clone(), rvar.clone()
            got = ops.BnGeluFn.apply(ui, wi, bi, rm2, rv2, 0.1, 1e-5)
            assert torch.equal(got, z) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
            got.backward(g)
            for leaf, q, w_ in zip((ui, wi, bi), req, want):
                assert (leaf.grad is not None) == q
                assert leaf.grad is None or (torch.equal(leaf.grad, w_) and leaf.grad.dtype == leaf.dtype)
        for sc in (None, scale):
            rm, rv = rmean.clone(), rvar.clone()
            out, mean, invstd = ops.bn_add_train(u, r, weight, bias, sc, rm, rv, 0.1, 1e-5)
            want = ops.bn_add_train_backward(u, ga, weight, mean, invstd, sc)
            for req in ((True, True, True, True), (True, False, False, False), (False, True, False, False), (False, False, True, True), (False, True, False, True)):
                ui, ri, wi, bi = (t.detach().clone().requires_grad_(q) for t, q in zip((u, r, weight, bias), req))
                rm2, rv2 = rmean.clone(), rvar.clone()
                got = ops.BnAddFn.apply(ui, ri, sc, wi, bi, rm2, rv2, 0.1, 1e-5)
                assert got.dtype == rdt and torch.equal(got, out) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
                got.backward(ga)
                for leaf, q, w_ in zip((ui, ri, wi, bi), req, (want[0], ga, want[1], want[2])):
                    assert (leaf.grad is not None) == q
                    assert leaf.grad is None or (torch.equal(leaf.grad, w_) and leaf.grad.dtype == leaf.dtype)
    if dt != f32:                                                               # a float32 gz for a 16-bit u is converted; the parameters' dtype is kept
        ui, wi, bi = u.detach().clone().requires_grad_(True), weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        ops.BnGeluFn.apply(ui, wi, bi, None, None, 0.1, 1e-5).float().backward(g.float().contiguous())
        assert ui.grad.dtype == dt and wi.grad.dtype == f32


@pytest.mark.gpu
def test_gelu_function_saves_one_tensor_of_the_input_size_and_add_returns_the_gradient_itself():
    u, g, r, ga, scale, weight, bias, _, _ = _inputs((4, 32, 7, 7), torch.bfloat16, seed=3)
    packed = []

    def pack(t):
        packed.append(t)
        return t
    ui, wi, bi = u.clone().requires_grad_(True), weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        z = ops.BnGeluFn.apply(ui, wi, bi, None, None, 0.1, 1e-5)
    big = [t for t in packed if t.numel() == u.numel()]
    assert len(big) == 1 and big[0].data_ptr() == ui.data_ptr() and len(packed) == 5 and sorted(t.numel() for t in packed) == [32] * 4 + [u.numel()]
    z.backward(g)
    packed.clear()
    ri = r.clone().requires_grad_(True)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = ops.BnAddFn.apply(ui, ri, scale, wi, bi, None, None, 0.1, 1e-5)
    assert sum(t.numel() == u.numel() for t in packed) == 1                     # u; neither r nor the output
    out.backward(ga)
    assert torch.equal(ri.grad, ga)                                             # dL/dr is the incoming gradient, element for element


@pytest.mark.gpu
def test_one_value_per_channel_raises_as_torch_does():
    x = torch.randn(1, 8, 1, 1, device=DEV)
    w, b = torch.ones(8, device=DEV), torch.zeros(8, device=DEV)
    msg = "Expected more than 1 value per channel when training"
    with pytest.raises(ValueError, match=msg):
        ops.bn_gelu_train(x, w, b)
    with pytest.raises(ValueError, match=msg):
        ops.bn_add_train(x, x, w, b)
    with pytest.raises(ValueError, match=msg):
        ops.bn_gelu_train_backward(x, x, w, b, b, w)
    with pytest.raises(ValueError, match=msg):
        ops.bn_add_train_backward(x, x, w, b, w)
    seq = lsmodels.mlp(8, 16).to(DEV).train()                                   # a marked mixer leaves it to the chain, which raises torch's own error
    bnact.mark(seq, seq, True)
    mode = bnact.mixer_ready(seq, x)
    assert mode == "all"
    with pytest.raises(ValueError, match=msg):
        bnact.run_mixer(seq, x, x, None, mode)


# ---- the router -------------------------------------------------------------------------------------------------------------------------------------------

def _randomize(m, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=gen) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=gen) * 0.2)


def _count(monkeypatch):
    calls = {"gelu_fwd": 0, "gelu_bwd": 0, "add_fwd": 0, "add_bwd": 0}
    for key, name in (("gelu_fwd", "bn_gelu_train"), ("gelu_bwd", "bn_gelu_train_backward"), ("add_fwd", "bn_add_train"), ("add_bwd", "bn_add_train_backward")):
        def wrap(*a, _real=getattr(bnact, name), _key=key, **k):
            calls[_key] += 1
            return _real(*a, **k)
        monkeypatch.setattr(bnact, name, wrap)
    return calls


def _hosts():
    m_mixer = models.default_token_mixer("m")
    return {
        "t-block": (lambda: lsmodels.MetaNeXtBlock(128, 2, num_heads=1, stage=1), (4, 128, 28, 28), 1, 1, 1),
        "m-block": (lambda: models.MetaNeXtBlock(64, 2, nn.GELU, 2, 0.0, "m", m_mixer), (4, 64, 14, 14), 1, 1, 1),
        "ls-downsample": (lambda: lsmodels.Downsample(64, 128), (4, 64, 28, 28), 1, 1, 1),
        "m-downsample": (lambda: models.Downsample(32, 2, nn.GELU), (4, 32, 28, 28), 1, 1, 1),
        "ls-stem": (lambda: lsmodels.RecNextStem(3, 64, additional_activation=True), (4, 3, 64, 64), 1, 3, 0),
        "ls-stem-identity": (lambda: lsmodels.RecNextStem(3, 64), (4, 3, 64, 64), 1, 2, 0),
        "m-stem": (lambda: models.RecNextStem(3, 64), (4, 3, 64, 64), 1, 1, 0),
        "t-block-droppath": (lambda: lsmodels.MetaNeXtBlock(128, 2, num_heads=1, stage=1, drop_path=0.5), (8, 128, 28, 28), 1, 1, 1),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(_hosts()))
def test_routed_mixer_calls_the_operators(monkeypatch, which):
    make, shape, marked, gelus, adds = _hosts()[which]
    torch.manual_seed(3)
    mix = make()
    _randomize(mix, 4)
    mix = mix.to(DEV).to(memory_format=torch.channels_last).train()
    x = torch.randn(*shape, device=DEV).contiguous(memory_format=torch.channels_last)
    twin = copy.deepcopy(mix)
    assert models.use_fused_mixer_norms_train(mix, all_shapes=True) == marked and models.use_fused_mixer_norms_train(mix, all_shapes=True) == 0
    calls = _count(monkeypatch)
    seen = []
    real_add = bnact.BnAddFn.apply
    monkeypatch.setattr(bnact.BnAddFn, "apply", staticmethod(lambda *a: seen.append((a[1], a[2])) or real_add(*a)))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    torch.manual_seed(21)
    ya = twin(xa)
    assert not any(calls.values())                                             # nothing is rerouted unless asked for
    torch.manual_seed(21)                                                      # the same DropPath mask
    yb = mix(xb)
    assert calls == {"gelu_fwd": gelus, "gelu_bwd": 0, "add_fwd": adds, "add_bwd": 0}
    ya.square().mean().backward(), yb.square().mean().backward()
    assert calls == {"gelu_fwd": gelus, "gelu_bwd": gelus, "add_fwd": adds, "add_bwd": adds}
    assert yb.dtype == ya.dtype and torch.allclose(yb, ya, atol=1e-3, rtol=1e-3) and torch.allclose(xb.grad, xa.grad, atol=1e-4, rtol=1e-2)
    if which == "t-block-droppath":
        (r, scale), = seen
        dropped = (scale == 0).nonzero().flatten().tolist()
        assert scale is not None and scale.dtype == f32 and 0 < len(dropped) < shape[0] and set(scale.tolist()) == {0.0, 2.0}
        for i in dropped:
            assert torch.equal(yb[i], r[i])                                    # a dropped sample's rows are the residual's, exactly
    elif adds:
        assert seen[0][1] is None
    for (k, a), (_, b) in zip(twin.named_buffers(), mix.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(b) == 1, k
        else:
            assert torch.allclose(a, b, atol=1e-5, rtol=1e-4), k
    for (k, p), (_, q) in zip(twin.named_parameters(), mix.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if q.grad is not None:
            assert q.grad.dtype == q.dtype and q.grad.shape == q.shape and bool(torch.isfinite(q.grad).all()), k
            if "channel_mixer" in k or k.startswith("stem."):                 # the routed norms' parameters and the 1x1 convs in front of them (through gu)
                assert torch.allclose(q.grad, p.grad, atol=1e-4, rtol=1e-2), (k, float((q.grad - p.grad).abs().max()))
    mix.eval(), twin.eval()
    with torch.no_grad():
        assert torch.allclose(mix(x), twin(x), atol=1e-3, rtol=1e-3)
    assert calls == {"gelu_fwd": gelus, "gelu_bwd": gelus, "add_fwd": adds, "add_bwd": adds}


@pytest.mark.gpu
def test_every_fallback_condition_keeps_the_chain_bit_for_bit(monkeypatch):
    monkeypatch.setattr(bnact.BnGeluFn, "apply", staticmethod(lambda *a: pytest.fail("BnGeluFn ran in a fallback condition")))
    monkeypatch.setattr(bnact.BnAddFn, "apply", staticmethod(lambda *a: pytest.fail("BnAddFn ran in a fallback condition")))
    # the library's own convs are not bit-reproducible from one call to the next (one module called twice on one tensor differs in the last bit of
    # this very Downsample's output); its deterministic algorithms are, and only then does "bit for bit" say anything about the path taken
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    x = torch.randn(4, 32, 14, 14, device=DEV).contiguous(memory_format=torch.channels_last)
    img = torch.randn(4, 3, 32, 32, device=DEV).contiguous(memory_format=torch.channels_last)

    def pair(change, make=lambda: lsmodels.Downsample(32, 64, drop_path=0.25), seed=6):
        torch.manual_seed(seed)
        ref = make()
        _randomize(ref, seed)
        ref = ref.to(DEV).to(memory_format=torch.channels_last).train()
        change(ref)
        hip = copy.deepcopy(ref)
        assert models.use_fused_mixer_norms_train(hip, all_shapes=True) == 1
        return ref, hip

    def same(ref, hip, inp, grad=True, what=""):
        xa, xb = inp.clone().requires_grad_(grad), inp.clone().requires_grad_(grad)
        torch.manual_seed(8)
        ya = ref(xa)
        torch.manual_seed(8)
        yb = hip(xb)
        assert ya.dtype == yb.dtype and torch.equal(ya, yb), (what, float((ya.detach().double() - yb.detach().double()).abs().max()))
        if grad:
            ya.float().square().sum().backward(), yb.float().square().sum().backward()
            assert torch.equal(xa.grad, xb.grad), what
            for (k, p), (_, q) in zip(ref.named_parameters(), hip.named_parameters()):
                assert (p.grad is None) == (q.grad is None), k
                if p.grad is not None and ("channel_mixer" in k or ".norm." in k):     # (the library's strided convs' weight gradients are not part of this)
                    assert torch.equal(p.grad, q.grad), k
        for (k, p), (_, q) in zip(ref.state_dict().items(), hip.state_dict().items()):
            assert torch.equal(p, q), k

    def norms(m):
        host = m.channel_mixer if hasattr(m, "channel_mixer") else m.stem
        return [cn.norm for cn in host if isinstance(cn, layers.ConvNorm)]

    def freeze(m):
        for bn in norms(m):
            bn.eval()
            for p in bn.parameters():
                p.requires_grad_(False)

    def sync(m):
        if hasattr(m, "channel_mixer"):
            m.channel_mixer = nn.SyncBatchNorm.convert_sync_batchnorm(m.channel_mixer)
        else:
            m.stem = nn.SyncBatchNorm.convert_sync_batchnorm(m.stem)

    def no_momentum(m):
        for bn in norms(m):
            bn.momentum = None

    def tanh_gelu(m):
        (m.channel_mixer if hasattr(m, "channel_mixer") else m.stem)[1] = nn.GELU(approximate="tanh")

    stem = lambda: lsmodels.RecNextStem(3, 32, additional_activation=True)
    for what, change in (("eval", lambda m: m.eval()), ("frozen norms", freeze), ("eval-mode norms", lambda m: [bn.eval() for bn in norms(m)]),
                         ("SyncBatchNorm", sync), ("momentum=None", no_momentum)):
        same(*pair(change), x, what=what)
        same(*pair(change, make=stem), img, what=what + ", stem")
    same(*pair(tanh_gelu), x)                                                    # not the exact GELU
    same(*pair(lambda m: m.bfloat16()), x.bfloat16())                            # 16-bit parameters, with the 16-bit activation of their own step
    same(*pair(lambda m: m.bfloat16(), make=stem), img.bfloat16())
    same(*pair(lambda m: models.replace_batchnorm(m.eval()).train()), x)         # the replace_batchnorm'ed form: the ConvNorms are nn.Conv2d
    same(*pair(lambda m: models.replace_batchnorm(m.eval()).train(), make=stem), img)
    same(*pair(lambda m: m.double()), x.double())                                # a dtype the kernels do not take
    ref, hip = pair(lambda m: None)                                              # CPU: the chain
    same(ref.cpu(), hip.cpu(), x.cpu())
    ref, hip = pair(lambda m: None, make=stem)
    same(ref.cpu(), hip.cpu(), img.cpu())
    ref, hip = pair(lambda m: None)                                              # a layer replaced after the marking: no longer the very layers
    for m in (ref, hip):
        m.channel_mixer[2] = copy.deepcopy(m.channel_mixer[2])
    same(ref, hip, x)
    fired = []                                                                   # a forward hook on a ConvNorm, on the GELU or on the Sequential: the chain, and it fires
    for pick in (lambda m: m.channel_mixer[0], lambda m: m.channel_mixer[1], lambda m: m.channel_mixer):
        ref, hip = pair(lambda m: None)
        handle = pick(hip).register_forward_hook(lambda mod, inp, out: fired.append(type(mod).__name__))
        same(ref, hip, x, what="hooked")
        handle.remove()
    assert fired == ["ConvNorm", "GELU", "Sequential"]
    ref, hip = pair(lambda m: None, make=stem)
    handle = hip.stem[2].register_forward_pre_hook(lambda mod, inp: fired.append("pre"))
    same(ref, hip, img, what="hooked stem")
    handle.remove()
    assert fired[-1] == "pre"
    ref, hip = pair(lambda m: None)                                              # an unmarked module is untouched
    del hip.channel_mixer.__dict__[bnact.ATTR]
    same(ref, hip, x)
    # the inference-only fused channel mixer comes first: eval mode, the folded form, bf16
    ref, hip = pair(lambda m: models.replace_batchnorm(m.eval()), make=lambda: lsmodels.Downsample(64, 128))
    for m in (ref, hip):
        m.bfloat16()
        assert models.use_linear_pointwise(m) == 2 and models.use_fused_mlp(m) == 1
    models.use_fused_mixer_norms_train(hip, all_shapes=True)
    with torch.no_grad():
        xin = torch.randn(4, 64, 56, 56, device=DEV).bfloat16().contiguous(memory_format=torch.channels_last)
        assert torch.equal(ref(xin), hip(xin))


def _t_style(seed=0):
    """RecNeXt-T's widths, heads and ratios at depth (0, 1, 1, 1), ten classes: every kind of block the T / S / B step has, HIP token mixers."""
    torch.manual_seed(seed)
    net = lsmodels.create_model("recnext_t", depth=(0, 1, 1, 1), drop_path_rate=0.0, num_classes=10)
    _randomize(net, 11)
    return net.to(DEV).to(memory_format=torch.channels_last).train()


@pytest.mark.gpu
@pytest.mark.parametrize("compose", [False, True], ids=["alone", "with-fused-rep-conv-norm-and-hip-batchnorm"])
def test_one_training_step_routed_against_an_unrouted_twin(monkeypatch, compose):
    base = _t_style()
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(4, 3, 224, 224, device=DEV, generator=gen).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (4,), device=DEV, generator=gen)
    nets = {k: copy.deepcopy(base) for k in ("u32", "r32", "u16", "r16")}
    mixers, gelus = 3 + 3, 3 + 3 + 3                                           # three blocks and three Downsamples; their GELUs and the stem's three
    for k in ("r32", "r16"):
        assert models.use_fused_mixer_norms_train(nets[k], all_shapes=True) == mixers + 1
        if compose:
            assert models.use_fused_rep_train(nets[k], all_shapes=True) > 0 and models.use_fused_conv_norm_train(nets[k], all_shapes=True) > 0
            assert models.use_hip_batchnorm(nets[k], all_shapes=True) > 0
    calls = _count(monkeypatch)
    loss = {}
    for k, net in nets.items():
        before = dict(calls)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=k.endswith("16")):
            loss[k] = F.cross_entropy(net(x), y)
        loss[k].backward()
        ran = {n: calls[n] - before[n] for n in calls}
        want = (gelus, mixers) if k.startswith("r") else (0, 0)
        assert ran == {"gelu_fwd": want[0], "gelu_bwd": want[0], "add_fwd": want[1], "add_bwd": want[1]}, (k, ran)
    lv = {k: float(v.detach().double()) for k, v in loss.items()}
    print(f"  losses: {lv}")
    assert all(torch.isfinite(v) for v in loss.values())
    # the routed float32 step is no further from the unrouted float32 step than the unrouted bf16-autocast step is
    assert abs(lv["r32"] - lv["u32"]) <= abs(lv["u16"] - lv["u32"]), lv
    for k in ("r32", "r16"):
        twin = dict(nets["u" + k[1:]].named_parameters())
        for name, p in nets[k].named_parameters():
            assert (p.grad is None) == (twin[name].grad is None), (k, name)
            if p.grad is not None:
                assert p.grad.dtype == p.dtype and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), (k, name)
        for (name, a), (_, b) in zip(nets["u" + k[1:]].named_buffers(), nets[k].named_buffers()):
            if name.endswith("num_batches_tracked"):
                assert int(a) == int(b) == 1, (k, name)
    live = [n for n, p in nets["u32"].named_parameters() if p.grad is not None]
    cat = lambda net: torch.cat([dict(net.named_parameters())[n].grad.flatten().double() for n in live])
    assert float(F.cosine_similarity(cat(nets["u32"]), cat(nets["r32"]), dim=0)) >= 0.999
    print(f"  cosine to the float32 step's gradients: unrouted bf16 {float(F.cosine_similarity(cat(nets['u32']), cat(nets['u16']), dim=0)):.4f}, "
          f"routed bf16 {float(F.cosine_similarity(cat(nets['u32']), cat(nets['r16']), dim=0)):.4f}")
