"""GPU: the HIP BatchNorm (rcx_batchnorm_*, ops.batch_norm_train / _frozen / _backward, ops.BatchNormFn, batchnorm.HipBatchNorm2d).

1  every output, element by element, against the float64 reference of tests/bn64.py under its bounds (K = 24 units of u32, never raised): the nine
   shapes and a tensor whose pointer is only element-aligned, float32 / bf16 / f16, four input distributions, batch and frozen statistics, every NULL
   combination of the backward's outputs; each case's worst ratio is recorded;
2  repeat launches bit for bit; tests/guard.py's properties A - E for forward and backward (running statistics are in-out by contract, so those cases pass
   none), and with running statistics given only those 2 C floats of the inputs change;
3  BatchNormFn under torch.autograd against the direct calls; HipBatchNorm2d's fallbacks, torch.equal to nn.BatchNorm2d; the R = 1 error."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from recnext_amd import _lib, batchnorm, ops
from tests import bn64, guard

DEV = torch.device("cuda:0")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
GUARDED = tuple(guard.LIBRARY_MODULES) + ("recnext_amd.batchnorm",)
_DT_IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
# every shape and the unaligned tensor x every dtype x every distribution the dtype can hold (2 + 1e-3 N(0, 1) is float32 only)
CASES = [(s, u, dt, dist) for s, u in [(s, False) for s in bn64.SHAPES] + [(bn64.UNALIGNED, True)] for dt in DTYPES for dist in bn64.dists_of(dt)]


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
@pytest.mark.parametrize("shape,unaligned,dt,dist", CASES,
                         ids=["x".join(map(str, s)) + ("-unaligned" if u else "") + f"-{_DT_IDS[dt]}-{dist}" for s, u, dt, dist in CASES])
def test_every_output_against_float64(shape, unaligned, dt, dist, record_property):
    d = bn64.case(shape, dt, dist)
    n, c, h, w = shape
    x, gy = cl(d["x"], dt, unaligned), cl(d["gy"], dt, unaligned)
    weight, bias = _gpu(d, "weight", "bias")
    worst = {}
    f32 = torch.float32

    # batch statistics, with and without running buffers
    rm, rv = _gpu(d, "running_mean", "running_var")
    y, mean, invstd = ops.batch_norm_train(x, weight, bias, rm, rv, bn64.MOMENTUM, bn64.EPS)
    assert y.dtype == dt and y.shape == x.shape and batchnorm._dense_nhwc(y) and mean.dtype == invstd.dtype == f32 and mean.shape == invstd.shape == (c,)
    ref = bn64.forward_ref(d["x"], d["weight"], d["bias"], bn64.EPS, running_mean=d["running_mean"], running_var=d["running_var"])
    for name, got, odt in (("y", y, dt), ("save_mean", mean, f32), ("save_invstd", invstd, f32), ("running_mean", rm, f32), ("running_var", rv, f32)):
        worst[name] = bn64.check(got, ref[name], odt, f"{shape} {dt} {dist} {name}")
    y2, mean2, invstd2 = ops.batch_norm_train(x, weight, bias, None, None, bn64.MOMENTUM, bn64.EPS)
    assert torch.equal(y2, y) and torch.equal(mean2, mean) and torch.equal(invstd2, invstd)

    # its backward from the kernel's own saved statistics: every NULL combination
    refb = bn64.backward_ref(d["x"], d["gy"], d["weight"], mean, invstd, True)
    full = ops.batch_norm_backward(x, gy, weight, mean, invstd, True)
    assert full[0].dtype == dt and batchnorm._dense_nhwc(full[0]) and full[1].dtype == full[2].dtype == f32
    for name, got, odt in (("gx", full[0], dt), ("gweight", full[1], f32), ("gbias", full[2], f32)):
        worst[name] = bn64.check(got, refb[name], odt, f"{shape} {dt} {dist} {name}")

    # frozen statistics
    rm0, rv0 = _gpu(d, "running_mean", "running_var")
    yf, invf = ops.batch_norm_frozen(x, weight, bias, rm0, rv0, bn64.EPS)
    reff = bn64.forward_ref(d["x"], d["weight"], d["bias"], bn64.EPS, mean=d["running_mean"], var=d["running_var"])
    worst["y_frozen"] = bn64.check(yf, reff["y"], dt, f"{shape} {dt} {dist} frozen y")
    r64 = 1.0 / torch.sqrt(d["running_var"].double() + float(torch.tensor(bn64.EPS, dtype=f32)))
    worst["invstd_frozen"] = bn64.check(invf, (r64, r64), f32, f"{shape} {dt} {dist} frozen invstd")
    reffb = bn64.backward_ref(d["x"], d["gy"], d["weight"], rm0, invf, False)
    fullf = ops.batch_norm_backward(x, gy, weight, rm0, invf, False)
    for name, got, odt in (("gx", fullf[0], dt), ("gweight", fullf[1], f32), ("gbias", fullf[2], f32)):
        worst[name + "_frozen"] = bn64.check(got, reffb[name], odt, f"{shape} {dt} {dist} frozen {name}")

    for batch, whole, m, r in ((True, full, mean, invstd), (False, fullf, rm0, invf)):
        for need_x, need_p in ((True, False), (False, True)):
            part = ops.batch_norm_backward(x, gy, weight, m, r, batch, need_input_grad=need_x, need_param_grads=need_p)
            assert (part[0] is None) == (not need_x) and (part[1] is None) == (part[2] is None) == (not need_p)
            for got, want in zip(part, whole):
                assert got is None or torch.equal(got, want), (batch, need_x, need_p)
    with pytest.raises(ValueError):
        ops.batch_norm_backward(x, gy, weight, mean, invstd, True, need_input_grad=False, need_param_grads=False)
    record_property("worst_ratio", {k: round(v, 3) for k, v in worst.items()})
    print(f"  {shape} {dt} {dist}: worst err / u32 bound units: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def _inputs(shape, dt, seed=5):
    gen = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x = cl(torch.randn(n, c, h, w, generator=gen) + 0.5, dt)
    gy = cl(torch.randn(n, c, h, w, generator=gen), dt)
    vec = lambda s, o: (torch.randn(c, generator=gen) * s + o).to(DEV)
    return x, gy, vec(0.5, 1.0), vec(0.3, 0.0), vec(0.2, 0.0), (torch.rand(c, generator=gen) + 0.5).to(DEV)


PROP_SHAPES = [(3, 21, 5, 9), (8, 40, 14, 14), (4, 768, 4, 4), (2, 16, 56, 56)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", PROP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_repeats_and_guard_bands(shape, dt):
    n, c, h, w = shape
    x, gy, weight, bias, rmean, rvar = _inputs(shape, dt)
    # A - D, and the repeat launch bit for bit (run_properties asserts it first), without running statistics: they are in-out by contract
    y, mean, invstd = guard.run_properties(lambda xx, ww, bb: ops.batch_norm_train(xx, ww, bb, None, None, 0.1, 1e-5), (x, weight, bias), modules=GUARDED)
    yf, invf = guard.run_properties(lambda xx, ww, bb, mm, vv: ops.batch_norm_frozen(xx, ww, bb, mm, vv, 1e-5), (x, weight, bias, rmean, rvar), modules=GUARDED)
    for batch, m, r in ((True, mean, invstd), (False, rmean, invf)):
        for need_x, need_p in ((True, True), (True, False), (False, True)):
            guard.run_properties(lambda xx, gg, ww, mm, rr: ops.batch_norm_backward(xx, gg, ww, mm, rr, batch, need_input_grad=need_x, need_param_grads=need_p),
                                 (x, gy, weight, m, r), modules=GUARDED)
    # E: the workspace is exactly as large as the query says, and the frozen backward without parameter gradients allocates none
    need = _lib.load().rcx_batchnorm_workspace_bytes(n, h, w, c, ops._DT[dt])
    for call, outs, has_ws in ((lambda: ops.batch_norm_train(x, weight, bias, None, None, 0.1, 1e-5), [x.numel() * x.element_size(), 4 * c, 4 * c], True),
                               (lambda: ops.batch_norm_backward(x, gy, weight, mean, invstd, True), [x.numel() * x.element_size(), 4 * c, 4 * c], True),
                               (lambda: ops.batch_norm_backward(x, gy, weight, rmean, invf, False, need_param_grads=False), [x.numel() * x.element_size()], False)):
        with guard.guarded_library(GUARDED) as rec:
            call()
            torch.cuda.synchronize()
            guard.check_guards(rec.arenas)
        ws = [a for a in rec.arenas if a.tensor.dtype == torch.uint8]
        assert ([a.nbytes for a in ws] == [need] and need > 0) if has_ws else not ws
        assert sorted(a.nbytes for a in rec.arenas if a.tensor.dtype != torch.uint8) == sorted(outs)

    # with running statistics given, only those 2 C floats of the inputs change
    for fill in (0x00, 0xFF):
        arenas = []
        gx_, gw_, gb_, gm_, gv_ = (guard.guarded_copy(t, fill, arenas) for t in (x, weight, bias, rmean, rvar))
        with guard.guarded_library(GUARDED) as rec:
            out = ops.batch_norm_train(gx_, gw_, gb_, gm_, gv_, 0.1, 1e-5)
            torch.cuda.synchronize()
            guard.check_guards(rec.arenas + arenas)
        guard.check_inputs_unchanged(arenas[:3])
        for a, old in zip(arenas[3:], (rmean, rvar)):
            changed = (a.buf != a.snapshot).nonzero().flatten()
            assert len(changed) and int(changed.min()) >= guard.GUARD and int(changed.max()) < guard.GUARD + 4 * c
            assert not torch.equal(a.tensor, old) and bool(torch.isfinite(a.tensor).all())
        guard.check_same(out, (y, mean, invstd), "running statistics given against none")

    def both_ways(xx, ww, bb, gg):
        xi, wi, bi = xx.detach().requires_grad_(True), ww.detach().requires_grad_(True), bb.detach().requires_grad_(True)
        out = ops.BatchNormFn.apply(xi, wi, bi, None, None, True, 0.1, 1e-5)
        return (out.detach(),) + torch.autograd.grad(out, (xi, wi, bi), gg)
    guard.run_properties(both_ways, (x, weight, bias, gy), modules=GUARDED)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_function_under_autograd_agrees_with_the_direct_calls(dt):
    shape = (5, 16, 13, 11)
    x, gy, weight, bias, rmean, rvar = _inputs(shape, dt, seed=9)
    for training in (True, False):
        if training:
            rm, rv = rmean.clone(), rvar.clone()
            y, mean, invstd = ops.batch_norm_train(x, weight, bias, rm, rv, 0.1, 1e-5)
        else:
            rm, rv, mean = rmean, rvar, rmean
            y, invstd = ops.batch_norm_frozen(x, weight, bias, rmean, rvar, 1e-5)
        want = ops.batch_norm_backward(x, gy, weight, mean, invstd, training)
        for req in ((True, True, True), (True, False, False), (False, True, True), (False, False, True)):
            xi, wi, bi = (t.detach().clone().requires_grad_(r) for t, r in zip((x, weight, bias), req))
            rm2, rv2 = rmean.clone(), rvar.clone()
            out = ops.BatchNormFn.apply(xi, wi, bi, rm2, rv2, training, 0.1, 1e-5)
            assert torch.equal(out, y) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
            out.backward(gy)
            for leaf, r, w_ in zip((xi, wi, bi), req, want):
                assert (leaf.grad is not None) == r
                assert leaf.grad is None or (torch.equal(leaf.grad, w_) and leaf.grad.dtype == leaf.dtype)
    # the parameters' gradients come back in the parameters' dtype; a float32 gy for a 16-bit x is converted
    if dt != torch.float32:
        xi, wi, bi = x.detach().clone().requires_grad_(True), weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        ops.BatchNormFn.apply(xi, wi, bi, None, None, True, 0.1, 1e-5).float().backward(gy.float().contiguous())
        assert xi.grad.dtype == dt and wi.grad.dtype == torch.float32


def _pair(c, **kw):
    torch.manual_seed(4)
    ref = nn.BatchNorm2d(c, **kw).to(DEV)
    if ref.affine:
        with torch.no_grad():
            ref.weight.uniform_(0.5, 1.5), ref.bias.uniform_(-0.3, 0.3)
    hip = batchnorm.HipBatchNorm2d(c, **kw).to(DEV)
    hip.hip_all_shapes = True                                                  # these shapes are smaller than the routing rule keeps
    hip.load_state_dict(ref.state_dict())
    return ref, hip


@pytest.mark.gpu
def test_module_takes_the_hip_path_and_matches_the_library(monkeypatch):
    calls = []
    real = batchnorm.BatchNormFn.apply
    monkeypatch.setattr(batchnorm.BatchNormFn, "apply", staticmethod(lambda *a: calls.append(a[5]) or real(*a)))
    ref, hip = _pair(24)
    x = torch.randn(4, 24, 7, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    for mode in ("train", "eval"):
        getattr(ref, mode)(), getattr(hip, mode)()
        xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        yr, yh = ref(xr), hip(xh)
        yr.square().sum().backward(), yh.square().sum().backward()
        assert torch.allclose(yh, yr, atol=2e-5, rtol=1e-5) and torch.allclose(xh.grad, xr.grad, atol=2e-4, rtol=1e-4)
        assert torch.allclose(hip.weight.grad, ref.weight.grad, atol=1e-3, rtol=1e-4) and torch.allclose(hip.bias.grad, ref.bias.grad, atol=1e-3, rtol=1e-4)
        assert torch.allclose(hip.running_mean, ref.running_mean, atol=1e-6) and torch.allclose(hip.running_var, ref.running_var, atol=1e-6)
        assert int(hip.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    assert calls == [True, False]
    with torch.autocast("cuda", dtype=torch.bfloat16):                         # a bf16 activation with float32 parameters: the autocast step's call
        ref.train(), hip.train()
        xb = x.bfloat16()
        yr, yh = ref(xb), hip(xb)
    assert yh.dtype == yr.dtype == torch.bfloat16 and torch.allclose(yh.float(), yr.float(), atol=4e-2, rtol=2e-2) and calls == [True, False, True]


@pytest.mark.gpu
def test_module_falls_back_to_the_library_unchanged(monkeypatch):
    monkeypatch.setattr(batchnorm.BatchNormFn, "apply", staticmethod(lambda *a: pytest.fail("the HIP path ran in a fallback condition")))
    x = torch.randn(4, 24, 7, 7, device=DEV)
    xcl = x.contiguous(memory_format=torch.channels_last)

    def same(ref, hip, inp, grad=False, view=lambda t: t):
        a, b = view(inp.clone()).requires_grad_(grad), view(inp.clone()).requires_grad_(grad)
        yr, yh = ref(a), hip(b)
        assert torch.equal(yr, yh) and yr.stride() == yh.stride()
        if grad:
            yr.square().sum().backward(), yh.square().sum().backward()
            assert torch.equal(a.grad, b.grad)
        for (k, p), (_, q) in zip(ref.state_dict().items(), hip.state_dict().items()):
            assert torch.equal(p, q), k

    ref, hip = _pair(24)
    ref.eval(), hip.eval()
    with torch.no_grad():
        same(ref, hip, xcl)                                                    # eval under no_grad
    for p in list(ref.parameters()) + list(hip.parameters()):
        p.requires_grad_(False)
    same(ref, hip, xcl)                                                        # eval, grad enabled, nothing wants a gradient
    ref, hip = _pair(24)
    same(ref, hip, x, grad=True)                                               # train, NCHW-strided input
    same(ref, hip, xcl, grad=True, view=lambda t: t[:, :, ::2])                # channels_last but not dense
    ref, hip = _pair(24)
    same(ref.cpu(), hip.cpu(), xcl.cpu(), grad=True)                           # CPU
    ref, hip = _pair(24)
    same(ref.bfloat16(), hip.bfloat16(), xcl.bfloat16(), grad=True)            # bf16 parameters
    ref, hip = _pair(24, momentum=None)
    same(ref, hip, xcl, grad=True)                                             # cumulative moving average
    ref, hip = _pair(24, affine=False)
    same(ref, hip, xcl, grad=True)                                             # no weight and bias
    ref, hip = _pair(24)
    same(ref.double(), hip.double(), xcl.double(), grad=True)                  # a dtype the kernels do not take
    ref, hip = _pair(24)
    x5 = torch.randn(4, 24, 7, device=DEV)
    with pytest.raises(ValueError):
        ref(x5)
    with pytest.raises(ValueError):
        hip(x5)                                                                # not 4-D: the parent's own error


@pytest.mark.gpu
def test_one_value_per_channel_raises_as_torch_does():
    ref, hip = _pair(8)
    x = torch.randn(1, 8, 1, 1, device=DEV)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ref(x)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        hip(x)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.batch_norm_train(x, hip.weight.detach(), hip.bias.detach())
    ref.eval(), hip.eval()
    xr, xh = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr, yh = ref(xr), hip(xh)                                                  # frozen statistics take one value per channel
    assert torch.allclose(yh, yr, atol=1e-6, rtol=1e-6)
