"""The classifier head on HIP (rcx_pool_head_fwd, rcx_global_pool_fwd; ops.pool_head, ops.global_pool, head.FusedHead after models.use_fused_head)
against float64 on the operands as the kernel sees them, with the per-element bound of tests/fwd64.py and grad64.K (tests/head64.py); bit-identity
across launches, batch sizes and batch positions; the five guard-band properties of tests/guard.py; the refusals; and the three model families.

Shapes (N, C, H, W, K): the smallest at which this kernel can go wrong -- ragged image tiles (N = 5, 3, 33, 2, 1 against tiles of 4), ragged class
tiles (K = 1000, 10, 7, 33, 1 against waves of 4 classes and tiles of 32), C that is no multiple of 64 (320, 448, 40), both channel paths (C <= 512,
and 640 > 512), a one-pixel plane and a non-square one.

Worst err / (u32 M) measured on the MI355X over the parity cases (16-bit: the part beyond half an ulp): see DESIGN.md section 5.z4."""
import functools

import pytest
import torch
import torch.nn as nn

from recnext_amd import _lib, head, models, ops
from tests import guard, head64
from tests.fwd64 import K, assert_fwd_close

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAMES = {F32: "f32", BF16: "bf16", F16: "f16"}
SHAPES = [(5, 512, 7, 7, 1000), (3, 640, 7, 7, 1000), (33, 320, 4, 4, 10), (2, 384, 16, 16, 1000), (3, 448, 5, 9, 7), (1, 64, 1, 1, 1), (4, 40, 2, 3, 33)]
MODULES = guard.LIBRARY_MODULES + ("recnext_amd.head",)


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _master(shape, kind):
    """float32 masters on the CPU, one set a (shape, kind): every dtype and weight type of a case rounds these."""
    n, c, h, w, k = shape
    g = torch.Generator(device="cpu").manual_seed(1000 * c + 10 * n + h)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(k, c, generator=g) * c ** -0.5
    b = torch.randn(k, generator=g) * 0.3
    if kind == "positive":
        x, wt, b = x.abs(), wt.abs(), b.abs()
    return x, wt, b


def _operands(shape, kind, dtype, wdtype):
    x, wt, b = _master(shape, kind)
    return x.to(dtype).to(dev()).contiguous(memory_format=torch.channels_last), wt.to(wdtype).to(dev()), b.to(dev())


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, dtype, wdtype, bias):
    x, wt, b = _master(shape, kind)
    return head64.pool_head_fwd64(x.to(dtype), wt.to(wdtype), b if bias else None)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=list(NAMES.values()))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_head_meets_the_float64_bound(shape, dtype, record_property):
    worst = {}
    for kind in ("random", "positive"):
        for wdtype in sorted({F32, dtype}, key=str):
            x, wt, b = _operands(shape, kind, dtype, wdtype)
            for bias in (True, False):
                got = ops.pool_head(x, wt, b if bias else None, shape[4])
                assert got.dtype == dtype and tuple(got.shape) == (shape[0], shape[4]) and got.is_contiguous()
                ref, mag = _reference(shape, kind, dtype, wdtype, bias)
                name = f"{kind} w={NAMES[wdtype]} bias={bias}"
                worst[name] = assert_fwd_close(got, ref, mag, dtype, name=name, layout="nk")
    record_property("worst_ratio", round(max(worst.values()), 3))
    print(f"\npool_head {shape} {NAMES[dtype]}: worst err / (u32 M) = {max(worst.values()):.3f} of K = {K}: " + ", ".join(f"{k}: {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=list(NAMES.values()))
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(map(str, s)))
def test_global_pool_meets_the_float64_bound(shape, dtype):
    worst = {}
    for kind in ("random", "positive"):
        x = _operands(shape, kind, dtype, dtype)[0]
        got = ops.global_pool(x)
        assert got.dtype == dtype and tuple(got.shape) == (shape[0], shape[1])
        ref, mag = head64.global_pool_fwd64(_master(shape, kind)[0].to(dtype))
        worst[kind] = assert_fwd_close(got, ref, mag, dtype, name=kind, layout="nc")
    print(f"\nglobal_pool {shape} {NAMES[dtype]}: worst err / (u32 M) = {max(worst.values()):.3f} of K = {K}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_repeat_launches_and_batch_positions_give_the_same_bits(dtype):
    """Row i of a batch of 33 == the image alone == the image in a batch of 5 (at another position of the image tile), and every launch the same."""
    shape = (33, 320, 4, 4, 10)
    for k, wdtype in ((10, dtype), (1000, F32)):
        x, wt, b = _operands(shape, "random", dtype, wdtype)
        if k != 10:
            g = torch.Generator(device="cpu").manual_seed(5)
            wt, b = (torch.randn(k, 320, generator=g) * 0.05).to(wdtype).to(dev()), torch.randn(k, generator=g).to(dev())
        full = ops.pool_head(x, wt, b, k)
        assert torch.equal(ops.pool_head(x, wt, b, k), full)
        pooled = ops.global_pool(x)
        assert torch.equal(ops.global_pool(x), pooled)
        for i in (0, 3, 6, 17, 32):
            one = x[i:i + 1].contiguous(memory_format=torch.channels_last)
            assert torch.equal(ops.pool_head(one, wt, b, k)[0], full[i]), (k, i)
            assert torch.equal(ops.global_pool(one)[0], pooled[i]), (k, i)
            lo = max(0, min(i - 1, 33 - 5))                                      # mostly another slot of the 4-image tile than in the batch of 33
            five = x[lo:lo + 5].contiguous(memory_format=torch.channels_last)
            assert torch.equal(ops.pool_head(five, wt, b, k)[i - lo], full[i]), (k, i, lo)
            assert torch.equal(ops.global_pool(five)[i - lo], pooled[i]), (k, i, lo)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 448, 5, 9, 7), (33, 320, 4, 4, 10)], ids=lambda s: "x".join(map(str, s)))
def test_guard_bands(shape, dtype):
    """Properties A - D of tests/guard.py (E: there is no workspace): nothing outside y written, every element of y written, nothing outside x, the weight
    and the bias read into the result, no input modified."""
    x, wt, b = _operands(shape, "random", dtype, dtype)
    k = shape[4]
    guard.run_properties(lambda xx, ww, bb: ops.pool_head(xx, ww, bb, k), (x, wt, b), modules=MODULES)
    guard.run_properties(lambda xx, ww: ops.pool_head(xx, ww, None, k), (x, wt.float()), modules=MODULES)
    guard.run_properties(lambda xx: ops.global_pool(xx), (x,), modules=MODULES)
    with guard.guarded_library(MODULES) as rec:                                  # the outputs do come out of this module's allocations
        ops.pool_head(x, wt, b, k), ops.global_pool(x)
        torch.cuda.synchronize()
    assert [tuple(a.tensor.shape) for a in rec.arenas] == [(shape[0], k), (shape[0], shape[1])]


def test_what_has_no_kernel_raises():
    x = torch.zeros(2, 12, 3, 3, device=dev()).contiguous(memory_format=torch.channels_last)
    with pytest.raises(_lib.RcxError):
        ops.pool_head(x, torch.zeros(5, 12, device=dev()), None, 5)              # C no multiple of 8
    with pytest.raises(_lib.RcxError):
        ops.global_pool(x)
    big = torch.zeros(1, 1032, 1, 1, device=dev()).contiguous(memory_format=torch.channels_last)
    with pytest.raises(_lib.RcxError):
        ops.pool_head(big, torch.zeros(5, 1032, device=dev()), None, 5)          # C above 1024
    ok = torch.zeros(2, 16, 3, 3, device=dev(), dtype=BF16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError):
        ops.pool_head(ok, torch.zeros(5, 16, device=dev(), dtype=F16), None, 5)  # a 16-bit weight of another type than x
    with pytest.raises(ValueError):
        ops.pool_head(ok, torch.zeros(5, 24, device=dev(), dtype=BF16), None, 5)
    with pytest.raises(ValueError):
        ops.pool_head(ok, torch.zeros(5, 16, device=dev(), dtype=BF16), torch.zeros(4, device=dev()), 5)
    with pytest.raises(ValueError):
        ops.pool_head(ok, torch.zeros(5, 16, dtype=BF16), None, 5)               # the weight on the CPU
    # NCHW strides are made channels_last by the wrapper, as every other entry does: same result
    g = torch.Generator(device="cpu").manual_seed(0)
    xn = torch.randn(2, 16, 3, 3, generator=g).to(dev())
    wt = torch.randn(5, 16, generator=g).to(dev())
    assert torch.equal(ops.pool_head(xn, wt, None, 5), ops.pool_head(xn.contiguous(memory_format=torch.channels_last), wt, None, 5))


# ---- the models ----------------------------------------------------------------------------------------------------------------------------------------------

def _stir(classifier, seed=3):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for nl in (classifier.head, classifier.head_dist):
            nl.norm.running_mean.copy_(torch.randn(nl.norm.running_mean.shape, generator=g) * 0.3)
            nl.norm.running_var.copy_(torch.rand(nl.norm.running_var.shape, generator=g) + 0.5)
            nl.norm.weight.copy_(torch.rand(nl.norm.weight.shape, generator=g) + 0.5)
            nl.norm.bias.copy_(torch.randn(nl.norm.bias.shape, generator=g) * 0.2)
            nl.linear.bias.copy_(torch.randn(nl.linear.bias.shape, generator=g) * 0.2)


@pytest.mark.parametrize("name", ["recnext_m0", "recnext_a0", "recnext_t"])
def test_model_head_route(name):
    from recnext_amd.speed import build_inference_model, synthetic_batch
    net = build_inference_model(name, dev(), BF16, seed=0)
    keys = list(net.state_dict())
    x = synthetic_batch(3, 224, dev(), BF16, seed=1)
    with torch.no_grad():
        feats = net.forward_features(x)
        plain = net.forward_head(feats)
        assert models.use_fused_head(net, all_shapes=True) == 1 and list(net.state_dict()) == keys
        assert net._fused_head.usable(net, feats)
        routed = net.forward_head(feats)
        assert torch.equal(net.forward_head(feats), routed)
    assert type(net.head) is nn.Linear and net._fused_head.packs()[0].data_ptr() == net.head.weight.data_ptr()
    ref, mag = head64.pool_head_fwd64(feats, net.head.weight, net.head.bias)
    worst = assert_fwd_close(routed, ref, mag, BF16, name=f"{name} routed head", layout="nk")
    print(f"\n{name}: routed head worst err / (u32 M) = {worst:.3f} of K = {K}; features {tuple(feats.shape)}")
    scale = float(plain.float().abs().max())
    diff = float((plain.float() - routed.float()).abs().max())
    assert diff < 0.05 * scale + 0.02, (diff, scale)
    # every fallback of a GPU tensor is the path as it was
    with torch.no_grad():
        nchw = feats.contiguous()
        if feats.shape[2] * feats.shape[3] > 1:
            assert not net._fused_head.usable(net, nchw)
        assert float((net.forward_head(nchw).float() - plain.float()).abs().max()) < 0.05 * scale + 0.02
    assert not net._fused_head.usable(net, feats)                                # grad enabled, the weight wants one
    net._fused_head.all_shapes = False
    with torch.no_grad():
        assert net._fused_head.usable(net, feats) == head.pool_head_routed(3, feats.shape[2], feats.shape[3], feats.shape[1], 1000, BF16)


@pytest.mark.parametrize("name", ["recnext_m0", "recnext_a0", "recnext_t"])
def test_model_unfused_classifier_route(name):
    """No replace_batchnorm: the eval-mode RecNextClassifier is folded and averaged in float32 at pack time; the bound is against its own float64 fold."""
    from recnext_amd.speed import build_inference_model, synthetic_batch
    from tests.test_head_cpu import _fold64
    torch.manual_seed(0)
    net = models.create_model(name, num_classes=1000).eval()
    _stir(net.head)
    net = net.to(device=dev(), dtype=BF16).to(memory_format=torch.channels_last).eval()
    x = synthetic_batch(3, 224, dev(), BF16, seed=1)
    with torch.no_grad():
        feats = build_inference_model(name, dev(), BF16, seed=0).forward_features(x)          # the inference trunk's features; the head under test is net's
        assert feats.is_contiguous(memory_format=torch.channels_last)
        plain = net.forward_head(feats)
        assert models.use_fused_head(net, all_shapes=True) == 1 and net._fused_head.usable(net, feats)
        routed = net.forward_head(feats)
        wpack, bias = net._fused_head.packs()
        assert wpack.dtype == F32 and bias.dtype == F32
        w64, b64, _, _ = _fold64(net.head)
    ref, mag = head64.pool_head_fwd64(feats, w64.cpu(), b64.cpu())
    worst = assert_fwd_close(routed, ref, mag, BF16, name=f"{name} unfused classifier", layout="nk")
    print(f"\n{name}: unfused-classifier head worst err / (u32 M) = {worst:.3f} of K = {K}")
    scale = float(plain.float().abs().max())
    assert float((plain.float() - routed.float()).abs().max()) < 0.05 * scale + 0.02
    net.train()
    with torch.no_grad():
        assert not net._fused_head.usable(net, feats)


def test_num_classes_zero_takes_the_pool():
    torch.manual_seed(0)
    net = models.replace_batchnorm(models.create_model("recnext_m0", num_classes=0)).eval().to(device=dev(), dtype=BF16).to(memory_format=torch.channels_last)
    assert type(net.head) is nn.Identity
    with torch.no_grad():
        feats = torch.randn(2, net.num_features, 7, 7, device=dev()).to(BF16).contiguous(memory_format=torch.channels_last)
        plain = net.forward_head(feats)
        assert models.use_fused_head(net, all_shapes=True) == 1 and net._fused_head.usable(net, feats)
        routed = net.forward_head(feats)
    assert routed.shape == plain.shape and routed.dtype == plain.dtype
    ref, mag = head64.global_pool_fwd64(feats)
    assert_fwd_close(routed, ref, mag, BF16, name="num_classes=0", layout="nc")


def test_graph_replay_of_a_routed_model_follows_a_head_weight_change():
    from recnext_amd.graph import GraphedInference
    from recnext_amd.speed import build_inference_model, synthetic_batch
    net = build_inference_model("recnext_m0", dev(), BF16, seed=0, fused_head=True)
    net._fused_head.all_shapes = True
    run = GraphedInference(net)
    x = synthetic_batch(2, 224, dev(), BF16, seed=0)
    with torch.no_grad():
        assert net._fused_head.usable(net, net.forward_features(x))
        want = net(x).clone()
        assert torch.equal(run(x), want)
        assert len(net._fused_head.packs()) == 2
        net.head.weight.mul_(2)                                                  # in place: the graph is captured again on the new weights
        want2 = net(x).clone()
        assert not torch.equal(want2, want)
        assert torch.equal(run(x), want2)
    assert len(run._graphs) == 1
