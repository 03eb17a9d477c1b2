"""GPU: the grouped 5x5 stride-2 Downsample conv of RecNeXt-T / S / B as one HIP launch (rcx_grouped_conv2d_fwd, ops.grouped_conv2d) against
F.conv2d in float64 on bf16-representable inputs and weights; repeat launches and batch shards bit for bit; guard bands; the Downsample module
after models.use_hip_downsample (folding, the library path where a gradient is wanted); the tiny models' fixtures, graph replay, the launch path
and two whole models.

Bars: float32 <= 2e-4 max(1, max|want|); bf16 / fp16 the bf16_bar of tests/test_lsnet_gpu.py (|d| <= 1e-2 + 1e-2 |want|).  The sums have 25 ci <= 100
float32 terms (relative error some 1e-6 of the sum of magnitudes) and a 16-bit output is rounded once (2^-9 relative), so both bars are far outside the
kernel's own error; float32 F.conv2d against the float64 one stays as far inside."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from recnext_amd import lsmodels, models, ops
from recnext_amd.graph import GraphedInference
from tests import guard
from tests.test_ls_down_cpu import ALL_NAMES
from tests.test_ls_share_cpu import load_tiny as load_share_tiny
from tests.test_ls_share_cpu import tiny as share_tiny
from tests.test_ls_share_gpu import _pair as share_pair
from tests.test_lsnet_cpu import _tiny
from tests.test_lsnet_gpu import _check_models, _pair, _randomize_bn, bf16_bar

DEV = torch.device("cuda:0")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)

# (N, H, W, Cin, Cout, G)
SHAPES = [
    (2, 7, 7, 48, 64, 16),            # 3 -> 4
    (2, 14, 14, 32, 48, 16),          # 2 -> 3
    (3, 9, 13, 16, 32, 16),           # 1 -> 2
    (1, 1, 1, 8, 12, 4),              # a single pixel
    (2, 2, 3, 6, 8, 2),               # smaller than one 5 x 5 window
    (1, 5, 6, 210, 280, 70),          # a ragged last wave
    (1, 37, 50, 64, 96, 32),          # several tiles each way
    (2, 28, 28, 128, 256, 128),       # the registered widths
    (2, 14, 14, 256, 384, 128),
    (2, 7, 7, 384, 512, 128),
    (2, 28, 28, 64, 128, 64),
    (2, 7, 7, 256, 512, 256),
]


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=None)
def case(shape):
    """(x, w, b, want with the bias, want without) on the CPU: bf16-representable float32 x, w and b, the float64 conv of them.  Made once a shape."""
    n, h, w_, cin, cout, g = shape
    gen = torch.Generator().manual_seed(hash(shape) % (1 << 31))
    ci = cin // g
    x = torch.randn(n, cin, h, w_, generator=gen).bfloat16().float()
    w = (torch.randn(cout, ci, 5, 5, generator=gen) / (25 * ci) ** 0.5).bfloat16().float()
    b = (0.5 * torch.randn(cout, generator=gen)).bfloat16().float()
    want0 = F.conv2d(x.double(), w.double(), None, stride=2, padding=2, groups=g)
    want = want0 + b.double().view(1, -1, 1, 1)
    return x, w, b, want, want0


def within(got, want, dt):
    got = got.double().cpu()
    err = float((got - want).abs().max())
    if dt == torch.float32:
        bar = 2e-4 * max(1.0, float(want.abs().max()))
        print(f"  {dt}: max|err| {err:.3e}, bar {bar:.3e}")
        return err <= bar
    print(f"  {dt}: max|err| {err:.3e}, max|want| {float(want.abs().max()):.3e}")
    return bf16_bar(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_float64_conv(shape, dt):
    n, h, w_, cin, cout, g = shape
    x, w, b, want, want0 = case(shape)
    xg = cl(x).to(dt)
    wp = ops.pack_grouped_weight(w.to(DEV))
    assert ops.grouped_conv2d_supported(n, h, w_, cin, cout, g, 5, 2, dt)
    y = ops.grouped_conv2d(xg, wp, b.to(DEV), g)
    y0 = ops.grouped_conv2d(xg, wp, None, g)
    for out in (y, y0):
        assert out.dtype == dt and tuple(out.shape) == (n, cout, (h + 1) // 2, (w_ + 1) // 2)
        assert out.permute(0, 2, 3, 1).is_contiguous()
    assert within(y, want, dt)
    assert within(y0, want0, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("plane", [(7, 7, 48, 64, 16), (14, 14, 256, 384, 128)], ids=lambda s: "x".join(map(str, s)))
def test_repeat_launches_and_batch_shards_are_bit_identical(plane, dt):
    h, w_, cin, cout, g = plane
    gen = torch.Generator().manual_seed(11)
    x = cl(torch.randn(6, cin, h, w_, generator=gen)).to(dt)
    wp = ops.pack_grouped_weight((torch.randn(cout, cin // g, 5, 5, generator=gen) / 5).to(DEV))
    b = torch.randn(cout, generator=gen).to(DEV)
    y = ops.grouped_conv2d(x, wp, b, g)
    for _ in range(5):
        assert torch.equal(ops.grouped_conv2d(x, wp, b, g), y)
    singles = torch.cat([ops.grouped_conv2d(x[i:i + 1], wp, b, g) for i in range(6)])
    assert torch.equal(singles, y)
    parts = torch.cat([ops.grouped_conv2d(x[a:e], wp, b, g) for a, e in ((0, 1), (1, 4), (4, 6))])
    assert torch.equal(parts, y)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(2, 9, 13, 16, 32, 16), (2, 7, 7, 384, 512, 128)], ids=lambda s: "x".join(map(str, s)))
def test_guard_bands_of_the_entry(shape, dt):
    n, h, w_, cin, cout, g = shape
    gen = torch.Generator().manual_seed(5)
    x = cl(torch.randn(n, cin, h, w_, generator=gen)).to(dt)
    wp = ops.pack_grouped_weight((torch.randn(cout, cin // g, 5, 5, generator=gen) / 5).to(DEV))
    b = torch.randn(cout, generator=gen).to(DEV)
    guard.run_properties(lambda xx, ww, bb: ops.grouped_conv2d(xx, ww, bb, g), (x, wp, b))
    guard.run_properties(lambda xx, ww: ops.grouped_conv2d(xx, ww, None, g), (x, wp))


def _downsample(cin, cout, seed=0):
    torch.manual_seed(seed)
    m = lsmodels.Downsample(cin, cout).eval()
    _randomize_bn(m)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_guard_bands_through_a_downsample_module(dt):
    """The module's own forward with the channel mixer taken out (y = t + t): the conv library's 1x1 convs are not bit-repeatable in float32
    (tests/test_ls_share_gpu.py), and properties A - D compare bits."""
    m = _downsample(48, 64)
    m.channel_mixer = torch.nn.Identity()
    assert models.use_hip_downsample(m) == 1
    m = m.to(DEV).to(dt).requires_grad_(False)
    x = cl(torch.randn(2, 48, 9, 13, generator=torch.Generator().manual_seed(3))).to(dt)
    calls = []
    real = ops.grouped_conv2d
    try:
        ops.grouped_conv2d = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
        with torch.no_grad():
            guard.run_properties(lambda xx: m(xx), (x,))
    finally:
        ops.grouped_conv2d = real
    assert len(calls) >= 5                                   # every call of run_properties went through the launch


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("cin,cout", [(48, 64), (256, 384)])
def test_module_folded_unfolded_and_against_the_library_path(cin, cout, dt):
    """Bit-identity is the conv's: the two modules (float32 parameters) run the launch on torch.equal packs, so its output is the same bits for an
    input of any of the three types.  Behind it the unfolded module's channel mixer applies its BatchNorms as operators and the folded one's has them
    in its weights, and a module cast to a 16-bit type rounds folded and unfolded parameters differently, so whole modules are held to the bars."""
    lib_mod = _downsample(cin, cout, seed=cin).to(DEV)                         # untouched: the library operators, in float32
    hip_mod = copy.deepcopy(lib_mod)
    assert models.use_hip_downsample(hip_mod) == 1
    fused = models.replace_batchnorm(copy.deepcopy(hip_mod))
    assert isinstance(fused.token_mixer, torch.nn.Conv2d) and fused._hip is True
    side = 14 if cin == 256 else 9
    x = cl(torch.randn(3, cin, side, side, generator=torch.Generator().manual_seed(cout)).bfloat16().float())
    outs = []
    real = ops.grouped_conv2d
    try:
        ops.grouped_conv2d = lambda *a, **kw: (outs.append(real(*a, **kw)), outs[-1])[1]
        with torch.no_grad():
            want = lib_mod(x).double().cpu()
            want_t = lib_mod.token_mixer(x).double().cpu()
            assert not outs
            fa = ops.grouped_conv2d(x.to(dt), *hip_mod.packed_params(), hip_mod.token_mixer.conv.groups)
            fb = ops.grouped_conv2d(x.to(dt), *fused.packed_params(), fused.token_mixer.groups)
            del outs[:]
            a = copy.deepcopy(hip_mod).to(dt)(x.to(dt))
            b = copy.deepcopy(fused).to(dt)(x.to(dt))
            assert len(outs) == 2
    finally:
        ops.grouped_conv2d = real
    assert a.dtype == dt and b.dtype == dt and a.grad_fn is None
    assert torch.equal(fa, fb)
    if dt == torch.float32:
        assert torch.equal(outs[0], fa) and torch.equal(outs[1], fa)          # and inside the modules' own forwards
    print(f"Downsample({cin} -> {cout}) {dt}: conv")
    assert within(fa, want_t, dt)
    print(f"Downsample({cin} -> {cout}) {dt}: module, unfolded then folded")
    assert within(a, want, dt)
    assert within(b, want, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["input_grad", "train"])
def test_a_wanted_gradient_takes_the_library_path(how):
    """With x.requires_grad, or in train mode, the library operators run: the output has a grad_fn and dL/dx is the untouched module's.  Both run the
    same operators on the same values; the conv library's float32 kernels are not bit-repeatable from call to call (tests/test_ls_share_gpu.py), so
    'the same' is 1e-5 of the largest gradient, ten times a float32 sum's own rounding and far below any change of function."""
    lib_mod = _downsample(48, 64, seed=2).to(DEV)
    hip_mod = copy.deepcopy(lib_mod)
    assert models.use_hip_downsample(hip_mod) == 1
    if how == "train":
        lib_mod.train()
        hip_mod.train()
    else:
        lib_mod.requires_grad_(False)
        hip_mod.requires_grad_(False)
    x = cl(torch.randn(2, 48, 9, 9, generator=torch.Generator().manual_seed(4)))
    calls = []
    real = ops.grouped_conv2d
    grads = []
    try:
        ops.grouped_conv2d = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
        for m in (lib_mod, hip_mod):
            xi = x.clone().requires_grad_(True)
            y = m(xi)
            assert y.grad_fn is not None
            y.square().sum().backward()
            grads.append(xi.grad)
    finally:
        ops.grouped_conv2d = real
    assert not calls
    d = float((grads[0] - grads[1]).abs().max())
    print(f"{how}: max|dgrad| {d:.3e}, max|grad| {float(grads[0].abs().max()):.3e}")
    assert d <= 1e-5 * float(grads[0].abs().max())
    if how == "input_grad":
        with torch.no_grad():                                # and the same module takes the launch again once no gradient is wanted
            try:
                ops.grouped_conv2d = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
                hip_mod(x)
            finally:
                ops.grouped_conv2d = real
        assert len(calls) == 1


def _tiny_ls():
    import numpy as np
    import os
    from tests.util import GOLDEN
    d = np.load(os.path.join(GOLDEN, "ls_tiny_model.npz"))
    sd = {k[4:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd::")}
    net = _tiny()
    net.load_state_dict(sd, strict=True)
    return net, torch.from_numpy(d["x"]), torch.from_numpy(d["logits"]), torch.from_numpy(d["logits_fused"])


def _tiny_share():
    x, logits, logits_fused, sd = load_share_tiny()
    net = share_tiny()
    net.load_state_dict(sd, strict=True)
    return net, x, logits, logits_fused


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["ls", "share"])
def test_tiny_models_fixtures_graph_replay_and_weight_updates(family, monkeypatch):
    """The bar is the one tests/test_ls_share_gpu.py applies to its tiny model on the GPU, 1e-3 max(1, max|logits|); tests/test_lsnet_cpu.py holds
    ls_tiny_model.npz to 1e-5 on the CPU with every operator the reference's own, which a HIP float32 forward is not asked to meet anywhere."""
    net, x, logits, logits_fused = _tiny_ls() if family == "ls" else _tiny_share()
    assert models.use_hip_downsample(net) == 3
    net = net.to(DEV).to(memory_format=torch.channels_last).requires_grad_(False)
    calls = []
    real = ops.grouped_conv2d
    monkeypatch.setattr(ops, "grouped_conv2d", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    xs = cl(x)
    bar = lambda a: 1e-3 * max(1.0, float(a.abs().max()))
    with torch.no_grad():
        got = net(xs)
        assert len(calls) == 3
        print(f"{family}: max|err| {float((got.cpu() - logits).abs().max()):.3e}, bar {bar(logits):.3e}")
        assert float((got.cpu() - logits).abs().max()) < bar(logits)
        models.replace_batchnorm(net)
        got = net(xs)
        assert len(calls) == 6
        assert float((got.cpu() - logits_fused).abs().max()) < bar(logits_fused)
        # graph replay against the plain forward, bit for bit, the 1x1 convs on the GEMM library as in every served model (tests/test_ls_share_gpu.py)
        models.use_linear_pointwise(net)
        for m, xx in ((net, xs), (copy.deepcopy(net).bfloat16(), xs.bfloat16())):
            want = m(xx)
            run = GraphedInference(m)
            assert torch.equal(run(xx), want)
            assert torch.equal(run(xx), want)
            # an in-place change of a Downsample weight: the pack is rebuilt and the replay follows it
            m.stages[2].downsample.token_mixer.weight.mul_(1.25)
            after = m(xx)
            assert not torch.equal(after, want)
            assert torch.equal(run(xx), after)
            assert torch.equal(run(xx), after)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_NAMES)
def test_launch_path_three_launches_and_no_grouped_conv_module(name, monkeypatch):
    torch.manual_seed(0)
    net = models.create_model(name).eval()
    assert models.use_hip_downsample(net) == 3
    net = net.to(DEV).to(memory_format=torch.channels_last)
    calls = []
    real = ops.grouped_conv2d
    monkeypatch.setattr(ops, "grouped_conv2d", lambda *a, **kw: (calls.append(tuple(a[0].shape)), real(*a, **kw))[1])
    grouped = []
    hooks = [m.register_forward_hook(lambda mod, i, o: grouped.append(mod)) for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.groups > 1]
    assert len(hooks) > 3
    x = torch.randn(1, 3, 224, 224, device=DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    assert [c[2:] for c in calls] == [(28, 28), (14, 14), (7, 7)], calls
    assert not grouped, grouped
    # without the reroute the three grouped convs are modules the forward calls
    plain = models.create_model(name).eval().to(DEV).to(memory_format=torch.channels_last)
    hooks = [m.register_forward_hook(lambda mod, i, o: grouped.append(mod)) for m in plain.modules() if isinstance(m, torch.nn.Conv2d) and m.groups > 1]
    with torch.no_grad():
        plain(x)
    for h in hooks:
        h.remove()
    assert len(grouped) == 3 and len(calls) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["recnext_s", "recnext_t_share_channel"])
def test_full_model_with_the_hip_downsample(name, monkeypatch):
    ref, net = (share_pair if name.endswith("share_channel") else _pair)(name)
    assert models.use_hip_downsample(net) == 3
    ref, net = ref.to(DEV), net.to(DEV).to(memory_format=torch.channels_last)
    calls = []
    real = ops.grouped_conv2d
    monkeypatch.setattr(ops, "grouped_conv2d", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    x = torch.randn(2, 3, 224, 224, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    _check_models(ref, net, x)                                     # BatchNorms unfolded (the pack folds them); float32 and bf16
    assert len(calls) == 6
    models.replace_batchnorm(ref)
    models.replace_batchnorm(net)
    _check_models(ref, net, x)
    assert len(calls) == 12
