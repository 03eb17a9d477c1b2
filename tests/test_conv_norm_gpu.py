"""GPU: a depthwise ConvNorm on batch statistics as one HIP operator (rcx_dwconv_bn_train_*, ops.dwconv_bn_train / dwconv_bn_train_backward / DwConvBnFn,
models.use_fused_conv_norm_train).

1  every output, element by element, against the float64 reference of tests/conv64.py under its bounds (K = 24 units of u32, never raised): the four forms
   (3x3, 5x5, 5x5 stride 2, 5x5 on x + resize(a)), bn64's nine shapes, four more (N = 1, H = 1, W = 1, a multi-tile C) and a tensor whose pointer is only
   element-aligned; float32 / bf16 / f16; bn64's input distributions; with and without conv bias, with and without running buffers; one weight row zero
   (var u = 0), one gamma zero and one negative.  gb is exact zeros.  Each case's worst ratio is recorded;
2  repeat launches bit for bit and tests/guard.py's properties A - D on four shapes; each need_* combination; DwConvBnFn under autograd against the direct
   calls; R = 1;
3  a routed LsRecAttn2d calls the operator three times each way and a routed LinearAttention3 once; every fallback condition keeps the chain bit for bit;
   one training step of a T-style model, alone and together with the fused RepVGGDW and the HIP BatchNorm."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from recnext_amd import _lib, batchnorm, dwbn, lsmodels, models, ops, recattn
from tests import bn64, conv64, guard
from tests.test_batchnorm_gpu import DEV, DTYPES, _DT_IDS, cl
from tests.test_repdw_gpu import _count as _count_rep
from tests.test_repdw_gpu import _randomize, _t_style

GUARDED = tuple(guard.LIBRARY_MODULES) + ("recnext_amd.batchnorm", "recnext_amd.repdw", "recnext_amd.dwbn")
_FORM_IDS = {f: "k%ds%d%s" % (f[0], f[1], "up" if f[2] else "") for f in conv64.FORMS}
CASES = [(f, s, u, dt, dist) for f in conv64.FORMS for s, u in [(s, False) for s in conv64.SHAPES] + [(bn64.UNALIGNED, True)] for dt in DTYPES
         for dist in bn64.dists_of(dt)]
HYPER = (conv64.MOM, conv64.EPS)
f32 = torch.float32


def _tensors(d, dt, unaligned, bias):
    x, g = cl(d["x"], dt, unaligned), cl(d["g"], dt, unaligned)
    a = cl(d["a"], f32, unaligned) if d["a"] is not None else None
    w, gamma, beta = (d[k].to(DEV) for k in ("w", "gamma", "beta"))
    return x, g, a, w, (d["b"].to(DEV) if bias else None), gamma, beta


@pytest.mark.gpu
@pytest.mark.parametrize("form,shape,unaligned,dt,dist", CASES,
                         ids=[_FORM_IDS[f] + "-" + "x".join(map(str, s)) + ("-unaligned" if u else "") + f"-{_DT_IDS[dt]}-{dist}" for f, s, u, dt, dist in CASES])
def test_every_output_against_float64(form, shape, unaligned, dt, dist, record_property):
    k, stride, up = form
    d = conv64.case(shape, dt, dist, form)
    n, c, h, w_ = shape
    ho, wo = conv64.out_hw(h, w_, stride)
    worst = {}
    for bias in (True, False):
        x, g, a, w, b, gamma, beta = _tensors(d, dt, unaligned, bias)
        tag = f"{form} {shape} {dt} {dist} bias={bias} "
        run = [d["running_mean"].to(DEV), d["running_var"].to(DEV)]
        y, stats, u = ops.dwconv_bn_train(x, w, b, gamma, beta, a, stride, run, *HYPER)
        assert y.dtype == dt and y.shape == (n, c, ho, wo) and batchnorm._dense_nhwc(y) and stats.dtype == f32 and stats.shape == (2, c)
        assert u.dtype == f32 and u.shape == y.shape and batchnorm._dense_nhwc(u)
        ref = conv64.forward_ref(d, form, bias=bias)
        got = {"y": y, "u": u, "mean_u": stats[0], "invstd_u": stats[1], "running_mean": run[0], "running_var": run[1]}
        for name, t in got.items():
            worst[name] = max(worst.get(name, 0.0), conv64.check(t, ref[name], dt if name == "y" else f32, tag + name))
        y2, stats2, u2 = ops.dwconv_bn_train(x, w, b, gamma, beta, a, stride, None, *HYPER)
        assert torch.equal(y2, y) and torch.equal(stats2, stats) and torch.equal(u2, u)          # the running buffers are written by the finalize alone

        refb = conv64.backward_ref(d, form, stats, bias=bias)
        gx, ga, grads = ops.dwconv_bn_train_backward(x, g, w, gamma, stats, u, a, stride)
        assert gx.dtype == dt and gx.shape == x.shape and batchnorm._dense_nhwc(gx) and len(grads) == 4 and all(t.dtype == f32 for t in grads)
        assert grads[0].shape == (c, 1, k, k) and all(t.shape == (c,) for t in grads[1:])
        assert (ga is None) == (not up) and (ga is None or (ga.dtype == f32 and ga.shape == a.shape and batchnorm._dense_nhwc(ga)))
        worst["gx"] = max(worst.get("gx", 0.0), conv64.check(gx, refb["gx"], dt, tag + "gx"))
        if up:
            worst["ga"] = max(worst.get("ga", 0.0), conv64.check(ga, refb["ga"], f32, tag + "ga"))
        for t, name in zip(grads, conv64.GRADS):
            worst[name] = max(worst.get(name, 0.0), conv64.check(t, refb[name], f32, tag + name))
        assert int(torch.count_nonzero(grads[1])) == 0                                             # gb: exactly zero, and inside its bound
    record_property("worst_ratio", {k_: round(v, 3) for k_, v in worst.items()})
    print("  " + f"{form} {shape} {dt} {dist} " + "worst err / u32 bound units: " + ", ".join(f"{k_} {v:.2f}" for k_, v in worst.items()))


def _inputs(shape, dt, form, seed=5, bias=True):
    k, stride, up = form
    gen = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    ho, wo = conv64.out_hw(h, w, stride)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x, g = cl(rn(n, c, h, w) + 0.5, dt), cl(rn(n, c, ho, wo), dt)
    a = cl(rn(n, c, *conv64.coarse_hw(h, w)), f32) if up else None
    par = [rn(c, 1, k, k) * 0.3, rn(c) * 0.2 if bias else None, rn(c) * 0.5 + 1.0, rn(c) * 0.3]
    run = [rn(c) * 0.2, torch.rand(c, generator=gen) + 0.5]
    return x, g, a, [None if t is None else t.to(DEV) for t in par], [t.to(DEV) for t in run]


def _flat(gx, ga, grads):
    return tuple(t for t in (gx, ga) + tuple(grads or ()) if t is not None)


PROP_SHAPES = [(3, 21, 5, 9), (8, 40, 14, 14), (4, 768, 4, 4), (2, 16, 56, 56)]
NEEDS = [(True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PROP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_repeats_and_guard_bands(shape, dt):
    n, c, h, w_ = shape
    for form in ((5, 2, False), (5, 1, True)) + (((3, 1, False),) if shape == PROP_SHAPES[0] else ()):
        k, stride, up = form
        x, g, a, par, run = _inputs(shape, dt, form)
        w, b, gamma, beta = par
        # A - D, and the repeat launch bit for bit (run_properties asserts it first); without running statistics, which are in-out by contract
        y, stats, u = guard.run_properties(lambda xx, aa, *pp: ops.dwconv_bn_train(xx, *pp, aa, stride, None, *HYPER), (x, a, *par), modules=GUARDED)
        full = None
        for need_x, need_a, need_p in NEEDS:
            if need_a and not up:
                continue
            out = guard.run_properties(lambda xx, gg, ss, uu, aa, ww, gm: ops.dwconv_bn_train_backward(
                xx, gg, ww, gm, ss, uu, aa, stride, need_input_grad=need_x, need_coarse_grad=need_a, need_param_grads=need_p),
                (x, g, stats, u, a, w, gamma), modules=GUARDED)
            assert (out[0] is None) == (not need_x) and (out[1] is None) == (not need_a) and (out[2] is None) == (not need_p)      # unrequested: unallocated
            if full is None:
                full = ops.dwconv_bn_train_backward(x, g, w, gamma, stats, u, a, stride)
            for got, want in zip(out[:2], full[:2]):
                assert got is None or torch.equal(got, want)
            assert out[2] is None or all(torch.equal(p_, q_) for p_, q_ in zip(out[2], full[2]))
        with pytest.raises(ValueError):
            ops.dwconv_bn_train_backward(x, g, w, gamma, stats, u, a, stride, need_input_grad=False, need_coarse_grad=False, need_param_grads=False)
        # with running statistics given, only those 2 C floats of the inputs change
        arenas = []
        gin = [None if t is None else guard.guarded_copy(t, 0xFF, arenas) for t in (x, a, *par)]
        nin = len(arenas)
        grun = [guard.guarded_copy(t, 0xFF, arenas) for t in run]
        with guard.guarded_library(GUARDED) as rec:
            out = ops.dwconv_bn_train(gin[0], *gin[2:], gin[1], stride, grun, *HYPER)
            torch.cuda.synchronize()
            guard.check_guards(rec.arenas + arenas)
        guard.check_inputs_unchanged(arenas[:nin])
        for ar, old in zip(arenas[nin:], run):
            changed = (ar.buf != ar.snapshot).nonzero().flatten()
            assert len(changed) and int(changed.min()) >= guard.GUARD and int(changed.max()) < guard.GUARD + 4 * c
            assert not torch.equal(ar.tensor, old) and bool(torch.isfinite(ar.tensor).all())
        guard.check_same(out, (y, stats, u), "running statistics given against none")

        def both_ways(xx, gg, aa, ww, bb, gm, bt):
            leaves = [t.detach().requires_grad_(True) for t in (xx, aa, ww, bb, gm, bt) if t is not None]
            it = iter(leaves)
            args = [next(it) if t is not None else None for t in (xx, aa, ww, bb, gm, bt)]
            o = ops.DwConvBnFn.apply(*args, None, None, stride, *HYPER)
            return (o.detach(),) + torch.autograd.grad(o, leaves, gg)
        guard.run_properties(both_ways, (x, g, a, *par), modules=GUARDED)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [(5, 2, False), (5, 1, True), (3, 1, False)], ids=lambda f: _FORM_IDS[f])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_function_under_autograd_agrees_with_the_direct_calls(dt, form):
    k, stride, up = form
    x, g, a, par, run = _inputs((5, 16, 13, 11), dt, form, seed=9)
    w, b, gamma, beta = par
    run0 = [t.clone() for t in run]
    y, stats, u = ops.dwconv_bn_train(x, w, b, gamma, beta, a, stride, run0, *HYPER)
    gx, ga, grads = ops.dwconv_bn_train_backward(x, g, w, gamma, stats, u, a, stride)
    want = (gx, ga) + grads
    for req in ((True,) * 6, (True,) + (False,) * 5, (False,) + (True,) * 5, (False, True, False, False, False, False), (False, False, False, True, False, True)):
        leaves = [None if t is None else t.detach().clone().requires_grad_(q) for t, q in zip([x, a] + par, req)]
        run1 = [t.clone() for t in run]
        if not any(l is not None and l.requires_grad for l in leaves):
            continue
        out = ops.DwConvBnFn.apply(*leaves, *run1, stride, *HYPER)
        assert torch.equal(out, y) and all(torch.equal(p_, q_) for p_, q_ in zip(run1, run0))
        out.backward(g)
        for leaf, q, w_ in zip(leaves, req, want):
            if leaf is None:
                continue
            assert (leaf.grad is not None) == q
            assert leaf.grad is None or (torch.equal(leaf.grad, w_) and leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape)
    # no conv bias (the A family): no gradient slot for it; a 16-bit coarse plane gets its gradient in its own type
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in [x, a.to(torch.bfloat16) if up else None, w, None, gamma, beta]]
    out = ops.DwConvBnFn.apply(*leaves, None, None, stride, *HYPER)
    out.backward(g)
    assert leaves[0].grad.dtype == dt and leaves[2].grad.dtype == f32 and (not up or leaves[1].grad.dtype == torch.bfloat16)


@pytest.mark.gpu
def test_one_value_per_channel_raises_as_torch_does():
    x, g, a, par, run = _inputs((1, 8, 1, 1), f32, (3, 1, False))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.dwconv_bn_train(x, *par)
    x2, g2, a2, par2, run2 = _inputs((1, 8, 2, 2), f32, (5, 2, False))            # one value at the OUTPUT of the stride-2 conv
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.dwconv_bn_train(x2, *par2, None, 2)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.dwconv_bn_train_backward(x2, g2, par2[0], par2[2], torch.zeros(2, 8, device=DEV), g2.float(), None, 2)
    cn = lsmodels.ConvNorm(8, 8, kernel_size=5, padding=2, stride=2, groups=8).to(DEV).train()
    cn._fused_conv_norm_train = "all"
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        recattn._conv_norm_train(cn, x2, 2)


# ---- the router -------------------------------------------------------------------------------------------------------------------------------------------

def _count(monkeypatch):
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = dwbn.dwconv_bn_train, dwbn.dwconv_bn_train_backward

    def cf(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def cb(*a, **k):
        calls["bwd"] += 1
        return bwd(*a, **k)
    monkeypatch.setattr(dwbn, "dwconv_bn_train", cf)
    monkeypatch.setattr(dwbn, "dwconv_bn_train_backward", cb)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["LsRecAttn2d", "LinearAttention3", "RecAttn2d"])
def test_routed_mixer_calls_the_operator(monkeypatch, which):
    torch.manual_seed(3)
    if which == "LsRecAttn2d":
        mix, x, times = lsmodels.LsRecAttn2d(32, num_heads=1, stage=1), torch.randn(4, 32, 28, 28, device=DEV), 3
    elif which == "RecAttn2d":                                                  # the A family: no conv bias
        mix, x, times = recattn.RecAttn2d(64, num_heads=2, stage=2), torch.randn(4, 64, 14, 14, device=DEV), 3
    else:
        mix, x, times = lsmodels.LinearAttention3(128, num_heads=4), torch.randn(4, 128, 7, 7, device=DEV), 1
    _randomize(mix, 4)
    mix = mix.to(DEV).to(memory_format=torch.channels_last).train()
    x = x.contiguous(memory_format=torch.channels_last)
    twin = copy.deepcopy(mix)
    assert models.use_fused_conv_norm_train(mix, all_shapes=True) == times
    calls = _count(monkeypatch)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = twin(xa)
    assert calls == {"fwd": 0, "bwd": 0}                                       # nothing is rerouted unless asked for
    yb = mix(xb)
    assert calls == {"fwd": times, "bwd": 0}
    ya.square().mean().backward(), yb.square().mean().backward()
    assert calls == {"fwd": times, "bwd": times}
    assert torch.allclose(yb, ya, atol=1e-3, rtol=1e-3) and torch.allclose(xb.grad, xa.grad, atol=1e-4, rtol=1e-2)
    for (k, a), (_, b) in zip(twin.named_buffers(), mix.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(b) == 1, k
        else:
            assert torch.allclose(a, b, atol=1e-5, rtol=1e-4), k
    for (k, p), (_, q) in zip(twin.named_parameters(), mix.named_parameters()):
        assert q.grad is not None and q.grad.dtype == q.dtype and q.grad.shape == q.shape and bool(torch.isfinite(q.grad).all()), k
        if k.endswith("conv.bias") and "qk" not in k:
            assert int(torch.count_nonzero(q.grad)) == 0, k                    # exactly zero; the chain leaves rounding noise here
    mix.eval(), twin.eval()
    with torch.no_grad():
        assert torch.allclose(mix(x), twin(x), atol=1e-3, rtol=1e-3)
    assert calls == {"fwd": times, "bwd": times}


@pytest.mark.gpu
def test_every_fallback_condition_keeps_the_chain_bit_for_bit(monkeypatch):
    monkeypatch.setattr(dwbn.DwConvBnFn, "apply", staticmethod(lambda *a: pytest.fail("the fused operator ran in a fallback condition")))
    x = torch.randn(4, 32, 7, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    a = torch.randn(4, 32, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)

    def pair(change, seed=6):
        torch.manual_seed(seed)
        ref = lsmodels.ConvNorm(32, 32, kernel_size=5, padding=2, groups=32, bias=True)
        _randomize(ref, seed)
        ref = ref.to(DEV).train()
        change(ref)
        hip = copy.deepcopy(ref)
        hip._fused_conv_norm_train = "all"
        return ref, hip

    def same(ref, hip, inp, coarse=None, mode="nearest"):
        run = (lambda m, t, c: recattn._conv_norm_train(m, t, 1)) if coarse is None else (lambda m, t, c: recattn._upadd_conv_norm_train(m, t, c, mode))
        xa, xb = inp.clone().requires_grad_(True), inp.clone().requires_grad_(True)
        ca = cb = None
        if coarse is not None:
            ca, cb = coarse.clone().requires_grad_(True), coarse.clone().requires_grad_(True)
        ya, yb = run(ref, xa, ca), run(hip, xb, cb)
        assert torch.equal(ya, yb) and ya.dtype == yb.dtype
        ya.float().square().sum().backward(), yb.float().square().sum().backward()
        assert torch.equal(xa.grad, xb.grad) and (ca is None or torch.equal(ca.grad, cb.grad))
        for (k, p), (_, q) in zip(ref.named_parameters(), hip.named_parameters()):
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
        for (k, p), (_, q) in zip(ref.state_dict().items(), hip.state_dict().items()):
            assert torch.equal(p, q), k

    def freeze(m):
        m.norm.eval()
        for p in m.norm.parameters():
            p.requires_grad_(False)

    def sync(m):
        m.norm = nn.SyncBatchNorm.convert_sync_batchnorm(m.norm)

    def no_momentum(m):
        m.norm.momentum = None

    for change in (lambda m: m.norm.eval(), freeze, lambda m: m.eval(), sync, no_momentum):
        same(*pair(change), x)
        same(*pair(change), x, a)
    same(*pair(lambda m: m.norm.bfloat16()), x.bfloat16())                       # 16-bit parameters, with the 16-bit activation of their own step
    same(*pair(lambda m: m.conv.bfloat16()), x.bfloat16(), a)
    same(*pair(lambda m: None), x, a, mode="bilinear")                           # the operator resizes by nearest only
    # the folded nn.Conv2d form, marked by hand: the first branch of both functions
    ref, hip = pair(lambda m: None)
    ca, cb = ref.fuse(), hip.fuse()
    cb._fused_conv_norm_train = "all"
    same(ca, cb, x)
    same(ca, cb, x, a)
    # CPU: the chain's own refusal, not the operator
    ref, hip = pair(lambda m: None)
    with pytest.raises(_lib.RcxError):
        recattn._conv_norm_train(hip.cpu(), x.cpu(), 1)
    with pytest.raises(_lib.RcxError):
        recattn._upadd_conv_norm_train(hip, x.cpu(), a.cpu(), "nearest")
    # an unmarked module is untouched
    ref, hip = pair(lambda m: None)
    del hip._fused_conv_norm_train
    same(ref, hip, x)
    same(ref, hip, x, a)


@pytest.mark.gpu
@pytest.mark.parametrize("compose", [False, True], ids=["alone", "with-fused-rep-and-hip-batchnorm"])
def test_one_training_step_routed_against_an_unrouted_twin(monkeypatch, compose):
    base = _t_style()
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(4, 3, 224, 224, device=DEV, generator=gen).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (4,), device=DEV, generator=gen)
    nets = {k: copy.deepcopy(base) for k in ("u32", "r32", "u16", "r16")}
    ra = sum(isinstance(m, recattn.RecAttn2d) for m in base.modules())
    la3 = sum(isinstance(m, lsmodels.LinearAttention3) for m in base.modules())
    reps = sum(isinstance(m, lsmodels.RepVGGDW) for m in base.modules())
    hosts = 3 * ra + la3
    assert ra == 2 and la3 == 1
    for k in ("r32", "r16"):
        assert models.use_fused_conv_norm_train(nets[k], all_shapes=True) == hosts
        if compose:
            assert models.use_fused_rep_train(nets[k], all_shapes=True) == reps
            assert models.use_hip_batchnorm(nets[k], all_shapes=True) > 0
    calls = _count(monkeypatch)
    rep_calls = _count_rep(monkeypatch)
    loss = {}
    for k, net in nets.items():
        before, rep_before = dict(calls), dict(rep_calls)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=k.endswith("16")):
            loss[k] = F.cross_entropy(net(x), y)
        loss[k].backward()
        ran = (calls["fwd"] - before["fwd"], calls["bwd"] - before["bwd"])
        assert ran == ((hosts, hosts) if k.startswith("r") else (0, 0)), (k, ran)
        rep_ran = (rep_calls["fwd"] - rep_before["fwd"], rep_calls["bwd"] - rep_before["bwd"])
        assert rep_ran == ((reps, reps) if compose and k.startswith("r") else (0, 0)), (k, rep_ran)
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
    # bf16 autocast at batch 4 is too noisy for a bar of its own (tests/test_repdw_gpu.py): printed
    print(f"  cosine to the float32 step's gradients: unrouted bf16 {float(F.cosine_similarity(cat(nets['u32']), cat(nets['u16']), dim=0)):.4f}, "
          f"routed bf16 {float(F.cosine_similarity(cat(nets['u32']), cat(nets['r16']), dim=0)):.4f}")
