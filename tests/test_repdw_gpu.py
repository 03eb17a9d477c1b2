"""GPU: RepVGGDW on batch statistics as one HIP operator (rcx_repdw_train_*, ops.repdw_train / repdw_train_backward / RepDwFn,
models.use_fused_rep_train).

1  every output, element by element, against the float64 reference of tests/rep64.py under its bounds (K = 24 units of u32, never raised): bn64's nine
   shapes, four more (N = 1, H = 1, W = 1, a multi-tile C) and a tensor whose pointer is only element-aligned; float32 / bf16 / f16; bn64's input
   distributions; one channel's w1 zero and one negative.  gb3 and gb1 are exact zeros.  Each case's worst ratio is recorded;
2  repeat launches bit for bit and tests/guard.py's properties A - D on four shapes; RepDwFn under autograd against the direct calls; R = 1;
3  a routed MetaNeXtBlock calls the operator once each way; every fallback condition keeps the chain bit for bit; one training step of a T-style model."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from recnext_amd import batchnorm, lsmodels, models, ops, repdw
from tests import bn64, guard, rep64
from tests.test_batchnorm_gpu import DEV, DTYPES, _DT_IDS, cl

GUARDED = tuple(guard.LIBRARY_MODULES) + ("recnext_amd.batchnorm", "recnext_amd.repdw")
CASES = [(s, u, dt, dist) for s, u in [(s, False) for s in rep64.SHAPES] + [(bn64.UNALIGNED, True)] for dt in DTYPES for dist in bn64.dists_of(dt)]
HYPER = (rep64.MOM_A, rep64.EPS_A, rep64.MOM_B, rep64.EPS_B)
BWD_PARAMS = ("w3", "b3", "gamma_a", "w1", "gamma_b")


def _gpu(d, names):
    return [d[k].to(DEV) for k in names]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,unaligned,dt,dist", CASES,
                         ids=["x".join(map(str, s)) + ("-unaligned" if u else "") + f"-{_DT_IDS[dt]}-{dist}" for s, u, dt, dist in CASES])
def test_every_output_against_float64(shape, unaligned, dt, dist, record_property):
    d = rep64.case(shape, dt, dist)
    n, c, h, w = shape
    f32 = torch.float32
    x, g = cl(d["x"], dt, unaligned), cl(d["g"], f32, unaligned)
    par, run = _gpu(d, rep64.PARAMS), _gpu(d, rep64.RUNNING)
    worst = {}
    tag = f"{shape} {dt} {dist} "

    r, stats = ops.repdw_train(x, *par, run, *HYPER)
    assert r.dtype == f32 and r.shape == x.shape and batchnorm._dense_nhwc(r) and stats.dtype == f32 and stats.shape == (4, c)
    ref = rep64.forward_ref(d["x"], d, running=d)
    worst["r"] = rep64.check(r, ref["r"], f32, tag + "r")
    for i, name in enumerate(rep64.STATS):
        worst[name] = rep64.check(stats[i], ref[name], f32, tag + name)
    for t, name in zip(run, rep64.RUNNING):
        worst[name] = rep64.check(t, ref[name], f32, tag + name)
    r2, stats2 = ops.repdw_train(x, *par, None, *HYPER)
    assert torch.equal(r2, r) and torch.equal(stats2, stats)                   # the running buffers are written by the finalize alone

    bpar = _gpu(d, BWD_PARAMS)
    refb = rep64.backward_ref(d["x"], d["g"], d, stats)
    gx, grads = ops.repdw_train_backward(x, g, *bpar, stats, rep64.EPS_B)
    assert gx.dtype == dt and gx.shape == x.shape and batchnorm._dense_nhwc(gx) and len(grads) == 8 and all(t.dtype == f32 for t in grads)
    assert grads[0].shape == (c, 1, 3, 3) and grads[4].shape == (c, 1, 1, 1) and all(grads[i].shape == (c,) for i in (1, 2, 3, 5, 6, 7))
    worst["gx"] = rep64.check(gx, refb["gx"], dt, tag + "gx")
    for t, name in zip(grads, rep64.GRADS):
        worst[name] = rep64.check(t, refb[name], f32, tag + name)
    assert int(torch.count_nonzero(grads[1])) == 0 and int(torch.count_nonzero(grads[5])) == 0      # gb3, gb1: exactly zero, and inside their bounds
    for need_x, need_p in ((True, False), (False, True)):
        gx1, grads1 = ops.repdw_train_backward(x, g, *bpar, stats, rep64.EPS_B, need_input_grad=need_x, need_param_grads=need_p)
        assert (gx1 is None) == (not need_x) and (grads1 is None) == (not need_p)
        assert gx1 is None or torch.equal(gx1, gx)
        assert grads1 is None or all(torch.equal(a, b) for a, b in zip(grads1, grads))
    with pytest.raises(ValueError):
        ops.repdw_train_backward(x, g, *bpar, stats, rep64.EPS_B, need_input_grad=False, need_param_grads=False)
    record_property("worst_ratio", {k: round(v, 3) for k, v in worst.items()})
    print("  " + tag + "worst err / u32 bound units: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def _inputs(shape, dt, seed=5):
    gen = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    rn = lambda *s: torch.randn(*s, generator=gen)
    x, g = cl(rn(n, c, h, w) + 0.5, dt), cl(rn(n, c, h, w), torch.float32)
    par = [rn(c, 1, 3, 3) * 0.3, rn(c) * 0.2, rn(c) * 0.5 + 1.0, rn(c) * 0.3, rn(c, 1, 1, 1) * 0.5 + 1.0, rn(c) * 0.2, rn(c) * 0.5 + 1.0, rn(c) * 0.3]
    run = [rn(c) * 0.2, torch.rand(c, generator=gen) + 0.5, rn(c) * 0.2, torch.rand(c, generator=gen) + 0.5]
    return x, g, [t.to(DEV) for t in par], [t.to(DEV) for t in run]


def _bwd_of(par):
    return [par[i] for i in (0, 1, 2, 4, 6)]


def _flat(gx, grads):
    return tuple(t for t in (gx,) + tuple(grads or ()) if t is not None)


PROP_SHAPES = [(3, 21, 5, 9), (8, 40, 14, 14), (4, 768, 4, 4), (2, 16, 56, 56)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PROP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_repeats_and_guard_bands(shape, dt):
    n, c, h, w = shape
    x, g, par, run = _inputs(shape, dt)
    # A - D, and the repeat launch bit for bit (run_properties asserts it first); without running statistics, which are in-out by contract
    r, stats = guard.run_properties(lambda xx, *pp: ops.repdw_train(xx, *pp, None, *HYPER), (x, *par), modules=GUARDED)
    for need_x, need_p in ((True, True), (True, False), (False, True)):
        guard.run_properties(lambda xx, gg, ss, *pp: _flat(*ops.repdw_train_backward(xx, gg, *pp, ss, rep64.EPS_B, need_input_grad=need_x, need_param_grads=need_p)),
                             (x, g, stats, *_bwd_of(par)), modules=GUARDED)
    # with running statistics given, only those 4 C floats of the inputs change
    arenas = []
    gx_ = guard.guarded_copy(x, 0xFF, arenas)
    gpar = [guard.guarded_copy(t, 0xFF, arenas) for t in par]
    grun = [guard.guarded_copy(t, 0xFF, arenas) for t in run]
    with guard.guarded_library(GUARDED) as rec:
        out = ops.repdw_train(gx_, *gpar, grun, *HYPER)
        torch.cuda.synchronize()
        guard.check_guards(rec.arenas + arenas)
    guard.check_inputs_unchanged(arenas[:9])
    for a, old in zip(arenas[9:], run):
        changed = (a.buf != a.snapshot).nonzero().flatten()
        assert len(changed) and int(changed.min()) >= guard.GUARD and int(changed.max()) < guard.GUARD + 4 * c
        assert not torch.equal(a.tensor, old) and bool(torch.isfinite(a.tensor).all())
    guard.check_same(out, (r, stats), "running statistics given against none")

    def both_ways(xx, gg, *pp):
        xi = xx.detach().requires_grad_(True)
        pi = [t.detach().requires_grad_(True) for t in pp]
        out = ops.RepDwFn.apply(xi, *pi, None, None, None, None, *HYPER)
        return (out.detach(),) + torch.autograd.grad(out, [xi] + pi, gg)
    guard.run_properties(both_ways, (x, g, *par), modules=GUARDED)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_function_under_autograd_agrees_with_the_direct_calls(dt):
    x, g, par, run = _inputs((5, 16, 13, 11), dt, seed=9)
    run0 = [t.clone() for t in run]
    r, stats = ops.repdw_train(x, *par, run0, *HYPER)
    gx, grads = ops.repdw_train_backward(x, g, *_bwd_of(par), stats, rep64.EPS_B)
    want = (gx,) + grads
    for req in ((True,) * 9, (True,) + (False,) * 8, (False,) + (True,) * 8, (False, False, False, True, False, False, True, False, False)):
        leaves = [t.detach().clone().requires_grad_(q) for t, q in zip([x] + par, req)]
        run1 = [t.clone() for t in run]
        out = ops.RepDwFn.apply(*leaves, *run1, *HYPER)
        assert torch.equal(out, r) and all(torch.equal(a, b) for a, b in zip(run1, run0))
        out.backward(g)
        for leaf, q, w_ in zip(leaves, req, want):
            assert (leaf.grad is not None) == q
            assert leaf.grad is None or (torch.equal(leaf.grad, w_) and leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape)
    leaves = [t.detach().clone().requires_grad_(True) for t in [x] + par]
    out = ops.RepDwFn.apply(*leaves, None, None, None, None, *HYPER)
    out.to(dt).backward(g.to(dt))                                             # a 16-bit cotangent reaches the operator as float32 through the cast's own backward
    assert leaves[0].grad.dtype == dt and leaves[1].grad.dtype == torch.float32


@pytest.mark.gpu
def test_one_value_per_channel_raises_as_torch_does():
    x, g, par, run = _inputs((1, 8, 1, 1), torch.float32)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.repdw_train(x, *par)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.repdw_train_backward(x, g, *_bwd_of(par), torch.zeros(4, 8, device=DEV))
    rep = lsmodels.RepVGGDW(8).to(DEV).train()
    models.use_fused_rep_train(rep, all_shapes=True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        lsmodels._rep_train(rep, x)


# ---- the router -------------------------------------------------------------------------------------------------------------------------------------------

def _randomize(m, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=gen) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=gen) * 0.2)


def _count(monkeypatch):
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = repdw.repdw_train, repdw.repdw_train_backward

    def cf(*a, **k):
        calls["fwd"] += 1
        return fwd(*a, **k)

    def cb(*a, **k):
        calls["bwd"] += 1
        return bwd(*a, **k)
    monkeypatch.setattr(repdw, "repdw_train", cf)
    monkeypatch.setattr(repdw, "repdw_train_backward", cb)
    return calls


@pytest.mark.gpu
def test_routed_block_calls_the_operator_once_each_way(monkeypatch):
    torch.manual_seed(3)
    block = lsmodels.MetaNeXtBlock(128, 2, num_heads=1, stage=1)
    _randomize(block, 4)
    block = block.to(DEV).to(memory_format=torch.channels_last).train()
    twin = copy.deepcopy(block)
    assert models.use_fused_rep_train(block, all_shapes=True) == 1
    calls = _count(monkeypatch)
    x = torch.randn(4, 128, 28, 28, device=DEV).contiguous(memory_format=torch.channels_last)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = twin(xa)
    assert calls == {"fwd": 0, "bwd": 0}                                       # nothing is rerouted unless asked for
    yb = block(xb)
    assert calls == {"fwd": 1, "bwd": 0}
    ya.square().mean().backward(), yb.square().mean().backward()
    assert calls == {"fwd": 1, "bwd": 1}
    assert torch.allclose(yb, ya, atol=1e-3, rtol=1e-3) and torch.allclose(xb.grad, xa.grad, atol=1e-4, rtol=1e-2)
    for (k, a), (_, b) in zip(twin.named_buffers(), block.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(a) == int(b) == 1, k
        elif "rep_mixer" in k:
            assert torch.allclose(a, b, atol=1e-5, rtol=1e-4), k
    for (k, p), (_, q) in zip(twin.named_parameters(), block.named_parameters()):
        assert q.grad is not None and q.grad.dtype == q.dtype and q.grad.shape == q.shape and bool(torch.isfinite(q.grad).all()), k
        if "rep_mixer" in k and "conv.bias" in k:
            assert int(torch.count_nonzero(q.grad)) == 0, k                    # exactly zero; the chain leaves rounding noise here
    block.eval(), twin.eval()
    with torch.no_grad():
        assert torch.allclose(block(x), twin(x), atol=1e-3, rtol=1e-3)
    assert calls == {"fwd": 1, "bwd": 1}


@pytest.mark.gpu
def test_every_fallback_condition_keeps_the_chain_bit_for_bit(monkeypatch):
    monkeypatch.setattr(repdw.RepDwFn, "apply", staticmethod(lambda *a: pytest.fail("the fused operator ran in a fallback condition")))
    x = torch.randn(4, 32, 7, 7, device=DEV).contiguous(memory_format=torch.channels_last)

    def pair(change, seed=6):
        torch.manual_seed(seed)
        ref = lsmodels.RepVGGDW(32)
        _randomize(ref, seed)
        ref = ref.to(DEV).train()
        change(ref)
        hip = copy.deepcopy(ref)
        assert models.use_fused_rep_train(hip, all_shapes=True) == 1
        return ref, hip

    def same(ref, hip, inp):
        a, b = inp.clone().requires_grad_(True), inp.clone().requires_grad_(True)
        ya, yb = lsmodels._rep_train(ref, a), lsmodels._rep_train(hip, b)
        assert torch.equal(ya, yb) and ya.dtype == yb.dtype
        ya.float().square().sum().backward(), yb.float().square().sum().backward()
        assert torch.equal(a.grad, b.grad)
        for (k, p), (_, q) in zip(ref.named_parameters(), hip.named_parameters()):
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k
        for (k, p), (_, q) in zip(ref.state_dict().items(), hip.state_dict().items()):
            assert torch.equal(p, q), k

    def freeze(m):
        m.sk.norm.eval()
        for p in m.sk.norm.parameters():
            p.requires_grad_(False)

    def sync(m):
        m.lk.norm = nn.SyncBatchNorm.convert_sync_batchnorm(m.lk.norm)

    def no_momentum(m):
        m.lk.norm.momentum = None

    def no_buffers_on_one(m):
        m.sk.norm.running_mean = m.sk.norm.running_var = m.sk.norm.num_batches_tracked = None

    for change in (lambda m: m.lk.norm.eval(), freeze, lambda m: m.eval(), sync, no_momentum, no_buffers_on_one):
        same(*pair(change), x)
    same(*pair(lambda m: m.lk.norm.bfloat16()), x.bfloat16())                   # 16-bit parameters, with the 16-bit activation of their own step
    # the fused nn.Conv2d form, marked by hand: _rep_train's first branch
    ref, hip = pair(lambda m: None)
    ca, cb = ref.fuse(), hip.fuse()
    cb._fused_rep_train = "all"
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya, yb = lsmodels._rep_train(ca, a), lsmodels._rep_train(cb, b)
    ya.sum().backward(), yb.sum().backward()
    assert torch.equal(ya, yb) and torch.equal(a.grad, b.grad) and torch.equal(ca.weight.grad, cb.weight.grad)


def _t_style(seed=0):
    """RecNeXt-T's widths, heads and ratios at depth (0, 1, 1, 1), ten classes: every kind of block the T / S / B step has, HIP token mixers."""
    torch.manual_seed(seed)
    net = lsmodels.create_model("recnext_t", depth=(0, 1, 1, 1), drop_path_rate=0.0, num_classes=10)
    _randomize(net, 11)
    return net.to(DEV).to(memory_format=torch.channels_last).train()


@pytest.mark.gpu
def test_one_training_step_routed_against_an_unrouted_twin(monkeypatch):
    base = _t_style()
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(4, 3, 224, 224, device=DEV, generator=gen).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (4,), device=DEV, generator=gen)
    nets = {k: copy.deepcopy(base) for k in ("u32", "r32", "u16", "r16")}
    reps = sum(isinstance(m, lsmodels.RepVGGDW) for m in base.modules())
    for k in ("r32", "r16"):
        assert models.use_fused_rep_train(nets[k], all_shapes=True) == reps == 3
    calls = _count(monkeypatch)
    loss = {}
    for k, net in nets.items():
        before = dict(calls)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=k.endswith("16")):
            loss[k] = F.cross_entropy(net(x), y)
        loss[k].backward()
        ran = (calls["fwd"] - before["fwd"], calls["bwd"] - before["bwd"])
        assert ran == ((reps, reps) if k.startswith("r") else (0, 0)), (k, ran)
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
    # bf16 autocast at batch 4 is too noisy for a bar of its own: measured against the float32 step's gradients, cosine 0.772 unrouted and 0.846 routed; printed
    print(f"  cosine to the float32 step's gradients: unrouted bf16 {float(F.cosine_similarity(cat(nets['u32']), cat(nets['u16']), dim=0)):.4f}, "
          f"routed bf16 {float(F.cosine_similarity(cat(nets['u32']), cat(nets['r16']), dim=0)):.4f}")
