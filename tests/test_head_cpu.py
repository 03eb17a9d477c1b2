"""CPU: the classifier head (rcx_pool_head_fwd, rcx_global_pool_fwd; recnext_amd/head.py; models.use_fused_head) as far as it goes without a GPU: the
binding, every refusal, the support rule, the pack, the router and its fallbacks, and that the float64 bound of tests/head64.py sees the faults a head
kernel can have.  The kernel itself is held to that bound in tests/test_head_gpu.py."""
import copy
import ctypes

import pytest
import torch
import torch.nn as nn

from recnext_amd import _lib, head, lsmodels, lsshare, models, ops
from tests import head64
from tests.fwd64 import K, U32, assert_fwd_close
from tests.test_grad_bound_cpu import _rtz

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT = _lib.DTYPE_F32, _lib.DTYPE_BF16, _lib.DTYPE_F16
ENTRIES = ("rcx_pool_head_supported", "rcx_pool_head_fwd", "rcx_global_pool_fwd")


def P(v):
    return ctypes.c_void_p(v)


# far apart, aligned to 4096: no two of the ranges of any case below overlap
X, WP, B, Y = 1 << 40, 2 << 40, 3 << 40, 4 << 40


def test_symbols_are_bound_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.rcx_abi_version() == 7 == _lib.ABI_VERSION
    for name in ("pool_head", "global_pool", "pack_head", "pool_head_supported"):
        assert getattr(ops, name) is getattr(head, name)
    header = open(__file__.replace("tests/test_head_cpu.py", "include/recnext_amd.h")).read()
    doc = header[header.index("The classifier head behind the last block"):header.index("int rcx_pool_head_supported(")]
    assert "forward_head" in doc and "RecNextClassifier" in doc and "recattn.py:266-293" in doc and ":307-387" in doc


def _head(x=X, w=WP, b=B, y=Y, n=5, h=7, wd=7, c=512, k=1000, xdt=1, wdt=1):
    return _lib.load().rcx_pool_head_fwd(P(x) if x else None, P(w) if w else None, P(b) if b else None, P(y) if y else None, n, h, wd, c, k, xdt, wdt, None)


def _pool(x=X, y=Y, n=5, h=7, wd=7, c=512, dt=1):
    return _lib.load().rcx_global_pool_fwd(P(x) if x else None, P(y) if y else None, n, h, wd, c, dt, None)


def test_every_refusal_comes_before_any_hip_call():
    err = lambda: _lib.load().rcx_last_error()
    # -1: a NULL x / wpack / y (a NULL bias is allowed: see the support rule below, nothing to launch here)
    for kw in ({"x": 0}, {"w": 0}, {"y": 0}):
        assert _head(**kw) == -1 and b"null" in err(), kw
    # -1: a non-positive extent
    for kw in ({"n": 0}, {"h": 0}, {"wd": -1}, {"c": 0}, {"k": 0}, {"k": -5}):
        assert _head(**kw) == -1 and b"non-positive" in err(), kw
    # -1: an unknown dtype, of x or of the weight
    for kw in ({"xdt": 3}, {"xdt": -1}, {"wdt": 7}):
        assert _head(**kw) == -1 and b"unknown dtype" in err(), kw
    # -1: a misaligned pointer (x and the weight to 16 bytes, y to one element, the bias to 4)
    for kw in ({"x": X + 8}, {"w": WP + 2}, {"y": Y + 1}, {"y": Y + 2, "xdt": 0, "wdt": 0}, {"b": B + 2}):
        assert _head(**kw) == -1 and b"aligned" in err(), kw
    # -1: y aliasing an input, from either end of the range
    nb = 5 * 1000 * 2
    for kw in ({"y": X}, {"y": WP}, {"y": B}, {"y": X + 5 * 49 * 512 * 2 - 2}, {"y": WP - nb + 2}, {"y": B + 3998}):
        assert _head(**kw) == -1 and b"overlap" in err(), kw
    # -1: 2^31 or more elements in x, in the weight or in y
    for kw in ({"n": 1 << 20, "h": 64, "wd": 64, "c": 8}, {"k": 1 << 21, "c": 1024}, {"n": 1 << 16, "k": 1 << 15, "h": 1, "wd": 1, "c": 8}, {"h": 1 << 16, "wd": 1 << 15, "c": 8, "n": 1}):
        assert _head(**kw) == -1 and b"2^31" in err(), kw
    # -2: no kernel for the shape
    for kw in ({"c": 12}, {"c": 1032}, {"c": 2048}, {"xdt": 2, "wdt": 1}, {"xdt": 0, "wdt": 2}):
        assert _head(**kw) == -2, kw
    # the pool alone
    assert _pool(x=0) == -1 and _pool(y=0) == -1 and _pool(n=0) == -1 and _pool(c=-8) == -1 and _pool(dt=5) == -1
    assert _pool(x=X + 4) == -1 and _pool(y=Y + 1) == -1 and _pool(y=X + 64) == -1
    assert _pool(n=1 << 20, h=64, wd=64, c=8) == -1 and b"2^31" in err()
    assert _pool(c=12) == -2 and _pool(c=1032) == -2


def test_supported_answers_without_a_gpu():
    sup = _lib.load().rcx_pool_head_supported
    for c in (320, 384, 448, 512, 640, 8, 40, 64, 1024):
        for k in (1, 7, 10, 33, 100, 1000):
            for xdt in DT:
                for wdt in (0, xdt):
                    assert sup(256, 7, 7, c, k, xdt, wdt) == 1, (c, k, xdt, wdt)
    assert sup(1, 1, 1, 64, 1, 0, 0) == 1 and sup(3, 5, 9, 448, 7, 1, 1) == 1 and sup(32, 16, 16, 384, 1000, 1, 0) == 1 and sup(2048, 4, 4, 512, 1000, 1, 1) == 1
    for bad in ((1, 7, 7, 12, 10, 0, 0), (1, 7, 7, 1032, 10, 1, 1), (1, 7, 7, 512, 10, 1, 2), (1, 7, 7, 512, 10, 0, 1), (0, 7, 7, 512, 10, 0, 0), (1, 7, 7, 512, 0, 0, 0),
                (1, 7, 7, 512, 10, 3, 0), (1 << 20, 64, 64, 8, 10, 0, 0), (1, 7, 7, 1024, 1 << 21, 0, 0)):
        assert sup(*bad) == 0, bad
    assert ops.pool_head_supported(5, 7, 7, 512, 1000, BF16) and ops.pool_head_supported(5, 7, 7, 512, 1000, BF16, F32)
    assert not ops.pool_head_supported(5, 7, 7, 512, 1000, BF16, F16) and not ops.pool_head_supported(5, 7, 7, 512, 1000, torch.float64)
    # the routing rule is a subset of the support rule
    for (c, p, es), (lo, hi) in head.ROUTED.items():
        assert lo >= 1 and hi >= lo and ops.pool_head_supported(lo, 1, p, c, 1000, F32 if es == 4 else BF16)


def test_wrappers_refuse_what_the_gpu_must_not_find():
    x = torch.zeros(2, 64, 3, 3)
    with pytest.raises(_lib.RcxError):
        ops.pool_head(x, torch.zeros(10, 64), None, 10)                       # a CPU tensor
    with pytest.raises(_lib.RcxError):
        ops.global_pool(x)
    with pytest.raises(ValueError):
        ops.pool_head(x[0], torch.zeros(10, 64), None, 10)
    with pytest.raises(ValueError):
        ops.pool_head(x.double(), torch.zeros(10, 64), None, 10)
    with pytest.raises(ValueError):
        ops.global_pool(x.long())
    with pytest.raises(ValueError):
        ops.pack_head(torch.zeros(10, 64).t())                                # not contiguous
    with pytest.raises(ValueError):
        ops.pack_head(torch.zeros(10, 64), torch.zeros(11))
    with pytest.raises(ValueError):
        ops.pack_head(nn.Linear(4, 4))                                        # a module that is no unfused RecNextClassifier
    with pytest.raises(ValueError):
        ops.pack_head(models.RecNextClassifier(16, 4).train())


# ---- the pack -----------------------------------------------------------------------------------------------------------------------------------------------

def _stir(classifier, seed=3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for nl in (classifier.head, classifier.head_dist):
            nl.norm.running_mean.copy_(torch.randn(nl.norm.running_mean.shape, generator=g) * 0.3)
            nl.norm.running_var.copy_(torch.rand(nl.norm.running_var.shape, generator=g) + 0.5)
            nl.norm.weight.copy_(torch.rand(nl.norm.weight.shape, generator=g) + 0.5)
            nl.norm.bias.copy_(torch.randn(nl.norm.bias.shape, generator=g) * 0.2)
            nl.linear.weight.copy_(torch.randn(nl.linear.weight.shape, generator=g) * 0.1)
            nl.linear.bias.copy_(torch.randn(nl.linear.bias.shape, generator=g) * 0.2)
    return classifier


def _fold64(classifier):
    """The float64 fold-and-average and, for the bias, the magnitude of the sums behind it."""
    ws, bs, ms = [], [], []
    for nl in (classifier.head, classifier.head_dist):
        n, lin = nl.norm, nl.linear
        scale = n.weight.double() / torch.sqrt(n.running_var.double() + n.eps)
        shift = n.bias.double() - scale * n.running_mean.double()
        ws.append(lin.weight.double() * scale.view(1, -1))
        bs.append(lin.weight.double() @ shift + lin.bias.double())
        ms.append(lin.weight.double().abs() @ (n.bias.double().abs() + (scale * n.running_mean.double()).abs()) + lin.bias.double().abs())
    return (ws[0] + ws[1]) / 2, (bs[0] + bs[1]) / 2, (ws[0].abs() + ws[1].abs()) / 2, (ms[0] + ms[1]) / 2


def test_pack_of_an_unfused_classifier_is_the_float64_fold_rounded_to_float32():
    cls = _stir(models.RecNextClassifier(320, 37)).eval()
    with torch.no_grad():
        w64, b64, wm, bm = _fold64(cls)
        wpack, bias, key = ops.pack_head(cls)
        fused = copy.deepcopy(cls).fuse()
    assert wpack.dtype == F32 and bias.dtype == F32 and tuple(wpack.shape) == (37, 320) and tuple(bias.shape) == (37,) and wpack.is_contiguous()
    # every weight is a handful of float32 roundings (sqrt, divide, two products, an add, the halving is exact) away from the float64 value; the bias is a
    # float32 dot product of 320 terms
    assert bool(((wpack.double() - w64).abs() <= 8 * U32 * wm).all())
    assert bool(((bias.double() - b64).abs() <= K * U32 * bm).all())
    assert float((wpack - fused.weight.detach()).abs().max()) < 1e-6 and float((bias - fused.bias.detach()).abs().max()) < 1e-5          # RecNextClassifier.fuse()'s own arithmetic
    assert len(key) == 12 and ops.pack_head(cls)[2] == key


def test_pack_of_a_linear_is_the_weights_own_storage():
    for dt in (F32, BF16, F16):
        lin = nn.Linear(64, 10).to(dt)
        wpack, bias, key = ops.pack_head(lin.weight, lin.bias)
        assert wpack.data_ptr() == lin.weight.data_ptr() and wpack.dtype == dt and tuple(wpack.shape) == (10, 64) and not wpack.requires_grad
        assert bias.dtype == F32 and torch.equal(bias, lin.bias.detach().float())
        assert ops.pack_head(lin.weight, None)[1] is None
        assert key == ops.pack_head(lin.weight, lin.bias)[2]
        with torch.no_grad():
            lin.bias.add_(1)
        assert key != ops.pack_head(lin.weight, lin.bias)[2]


# ---- the router ---------------------------------------------------------------------------------------------------------------------------------------------

_LS_TINY = dict(embed_dim=(32, 64, 96, 128), depth=(1, 1, 2, 2), mlp_ratios=(2, 2, 2, 1.5), split_rates=(4, 4, 4, 4), num_classes=10)


def _builders():
    """Tiny models of the three model modules, their token mixers on library operators so that they run on the CPU."""
    from tests.ls_eager import eager_token_mixer
    from tests.ls_share_eager import eager_share_token_mixer
    return {
        "models": lambda **kw: models.RecNext(family="m", embed_dim=(8, 16, 32, 64), depth=(1, 1, 1, 1), token_mixer=lambda dim, stage: nn.Conv2d(dim, dim, 3, padding=1, groups=dim),
                                              **dict({"num_classes": 10}, **kw)),
        "lsmodels": lambda **kw: lsmodels.RecNext(token_mixer=eager_token_mixer, num_heads=(1, 1, 1, 2), **dict(_LS_TINY, **kw)),
        "lsshare": lambda **kw: lsshare.RecNext(token_mixer=eager_share_token_mixer, **dict(_LS_TINY, depth=(1, 1, 2, 6), **kw)),
    }


@pytest.mark.parametrize("name", ["recnext_m0", "recnext_a0", "recnext_t", "recnext_t_share_channel"])
def test_use_fused_head_leaves_the_state_dict_alone(name):
    net = models.create_model(name).eval()
    keys, params, buffers = list(net.state_dict()), {k: id(p) for k, p in net.named_parameters()}, {k: id(b) for k, b in net.named_buffers()}
    assert models.use_fused_head(net) == 1 and models.use_fused_head(net) == 0
    assert type(net.__dict__["_fused_head"]) is head.FusedHead and "_fused_head" not in dict(net.named_modules())
    assert list(net.state_dict()) == keys and {k: id(p) for k, p in net.named_parameters()} == params and {k: id(b) for k, b in net.named_buffers()} == buffers
    models.replace_batchnorm(net)
    assert not net._fused_head.usable(net, torch.zeros(1, 8, 1, 1))           # the helper describes the head that was replaced
    assert models.use_fused_head(net) == 1 and models.use_fused_head(net) == 0 and type(net.head) is nn.Linear and net._fused_head.head is net.head
    assert list(net.state_dict()) == list(models.replace_batchnorm(models.create_model(name).eval()).state_dict())
    assert models.use_fused_head(nn.Linear(3, 3)) == 0


@pytest.mark.parametrize("which", ["models", "lsmodels", "lsshare"])
def test_a_cpu_tensor_takes_the_path_as_it_was(which):
    torch.manual_seed(2)
    a = _builders()[which]().eval()
    b = copy.deepcopy(a)
    assert models.use_fused_head(b, all_shapes=True) == 1
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        assert not b._fused_head.usable(b, b.forward_features(x))
        assert torch.equal(a(x), b(x))
        models.replace_batchnorm(a), models.replace_batchnorm(b)
        assert models.use_fused_head(b, all_shapes=True) == 1              # replace_batchnorm replaced the head: a new helper for the nn.Linear
        assert torch.equal(a(x), b(x))


class _FakeGpu:
    """usable() on a host without a GPU: a tensor that says it is a dense channels_last GPU tensor; nothing is launched."""

    def __init__(self, t, cuda=True, channels_last=True, requires_grad=False):
        self.t, self.is_cuda, self._cl, self.requires_grad = t, cuda, channels_last, requires_grad
        self.shape, self.dtype, self.device = t.shape, t.dtype, t.device

    def dim(self):
        return self.t.dim()

    def data_ptr(self):
        return self.t.data_ptr() & ~15

    def is_contiguous(self, memory_format=torch.contiguous_format):
        return self._cl if memory_format == torch.channels_last else self.t.is_contiguous()


def test_usable_is_false_for_each_fallback(monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _FakeGpu)))
    net = _builders()["models"]().eval()
    models.replace_batchnorm(net)
    assert models.use_fused_head(net, all_shapes=True) == 1
    fh = net._fused_head
    feat = torch.randn(2, 64, 2, 2)
    with torch.no_grad():
        assert fh.usable(net, _FakeGpu(feat))                                 # the reference point: everything in order
        assert not fh.usable(net, _FakeGpu(feat.bfloat16()))                  # x of another type than the head's parameters: the module's own path (its error, or autocast's cast)
        assert not fh.usable(net, feat)                                       # a CPU tensor
        assert not fh.usable(net, _FakeGpu(feat, cuda=False))
        assert not fh.usable(net, _FakeGpu(feat, channels_last=False))        # NCHW strides
        assert not fh.usable(net, _FakeGpu(feat.double()))                    # a type the kernel does not take
        assert not fh.usable(net, _FakeGpu(torch.randn(2, 60, 2, 2)))         # C not a multiple of 8 / not the head's
        net.train()
        assert not fh.usable(net, _FakeGpu(feat))                             # training
        net.eval()
        net.global_pool = ""
        assert not fh.usable(net, _FakeGpu(feat))                             # no average pool
        net.global_pool = "avg"
        fh.all_shapes = False
        assert fh.usable(net, _FakeGpu(feat)) == head.pool_head_routed(2, 2, 2, 64, 10, F32)      # the routing rule decides
        fh.all_shapes = True
        old = net.head
        net.head = nn.Linear(64, 10)
        assert not fh.usable(net, _FakeGpu(feat))                             # a replaced head
        net.head = old
        assert fh.usable(net, _FakeGpu(feat))
    assert not fh.usable(net, _FakeGpu(feat))                                 # grad enabled and the head's weight wants one
    assert not fh.usable(net, _FakeGpu(feat, requires_grad=True))
    for p in net.head.parameters():
        p.requires_grad_(False)
    assert fh.usable(net, _FakeGpu(feat)) and not fh.usable(net, _FakeGpu(feat, requires_grad=True))


def test_usable_covers_the_unfused_classifier_and_num_classes_zero(monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _FakeGpu)))
    feat = _FakeGpu(torch.randn(2, 64, 2, 2))
    with torch.no_grad():
        net = _builders()["models"](distillation=True).eval()
        assert models.use_fused_head(net, all_shapes=True) == 1 and net._fused_head.usable(net, feat)
        net.head.head.norm.train()
        assert not net._fused_head.usable(net, feat)                          # a BatchNorm on batch statistics cannot be folded
        net.head.head.norm.eval()
        net.train()
        assert not net._fused_head.usable(net, feat)                          # distillation in train mode returns two heads: the module's own path
        net.eval()
        net.head.head.norm = nn.SyncBatchNorm(64).eval()
        assert not net._fused_head.usable(net, feat)                          # exact types only
        bare = _builders()["models"](num_classes=0).eval()
        assert models.use_fused_head(bare, all_shapes=True) == 1 and not bare._fused_head.usable(bare, feat)     # an unfused classifier of nn.Identity heads
        models.replace_batchnorm(bare)
        assert type(bare.head) is nn.Identity and models.use_fused_head(bare, all_shapes=True) == 1
        assert bare._fused_head.usable(bare, feat) and bare._fused_head.packs() == []


def test_pack_follows_the_buffers_and_a_load_state_dict():
    net = _builders()["models"]().eval()
    _stir(net.head)
    models.use_fused_head(net)
    fh = net._fused_head
    with torch.no_grad():
        w0, b0 = fh._operands()
        assert fh._operands()[0] is w0 and fh.packs()[0] is w0
        sd = copy.deepcopy(net.state_dict())
        net.head.head.norm.running_mean.add_(1)
        w1, b1 = fh._operands()
        assert w1 is not w0 and torch.equal(w1, w0) and not torch.equal(b1, b0)           # the mean moves the bias alone
        assert bool(((b1.double() - _fold64(net.head)[1]).abs() <= K * U32 * _fold64(net.head)[3]).all())
        net.load_state_dict(sd)
        w2, b2 = fh._operands()
        assert w2 is not w1 and torch.equal(w2, w0) and torch.equal(b2, b0)
        net.head.head_dist.linear.weight.mul_(2)
        assert not torch.equal(fh._operands()[0], w0)


# ---- the bound sees what it must ----------------------------------------------------------------------------------------------------------------------------

SHAPE = (5, 512, 7, 7, 1000)


def _operands(kind, dtype, seed=11):
    n, c, h, w, k = SHAPE
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(k, c, generator=g) * c ** -0.5
    b = torch.randn(k, generator=g) * 0.3
    if kind == "positive":
        x, wt, b = x.abs(), wt.abs(), b.abs()
    return x.to(dtype), wt.to(dtype), b


def _emulate(x, wt, b, dtype, fault=None):
    """A float32 head on the CPU: 8 pixel slices and a tree, the float32 reciprocal, 64 partial sums a class and a tree, the bias, one rounding."""
    n, c, h, w = x.shape
    px = x.float().reshape(n, c, h * w)
    count = h * w
    if fault == "dropped_pixel":
        px = px[:, :, :-1]
    if fault == "divisor":
        count -= 1
    pad = (-px.shape[2]) % 8
    sl = torch.cat([px, px.new_zeros(n, c, pad)], 2).reshape(n, c, -1, 8)
    s = sl[:, :, 0]
    for i in range(1, sl.shape[2]):
        s = s + sl[:, :, i]
    pooled = (((s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])) + ((s[..., 4] + s[..., 5]) + (s[..., 6] + s[..., 7]))) * torch.tensor(1.0 / count, dtype=F32)
    if fault == "pooled_bf16":
        pooled = pooled.bfloat16().float()
    prod = (pooled[:, None, :] * wt.float()[None]).reshape(n, wt.shape[0], c // 64, 64)
    part = prod[:, :, 0]
    for i in range(1, c // 64):
        part = part + prod[:, :, i]
    width = 64
    while width > 1:
        width //= 2
        part = part[..., :width] + part[..., width:]
    y = part[..., 0] + b
    if fault == "bias_twice":
        y = y + b
    return _rtz(y.double(), dtype) if fault == "truncating_store" else y.to(dtype)


@pytest.mark.parametrize("kind", ["random", "positive"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_the_bound_passes_a_clean_float32_head_and_sees_each_fault(kind, dtype):
    x, wt, b = _operands(kind, dtype)
    ref, mag = head64.pool_head_fwd64(x, wt, b)
    worst = assert_fwd_close(_emulate(x, wt, b, dtype), ref, mag, dtype, name=f"clean {kind}")
    print(f"clean float32 head, {kind}, {dtype}: worst err / (u32 M) = {worst:.2f}")
    assert worst < K / 4
    faults = ["pooled_bf16", "dropped_pixel", "divisor", "bias_twice"] + (["truncating_store"] if dtype != F32 else [])
    for fault in faults:
        with pytest.raises(AssertionError, match="outside the bound"):
            assert_fwd_close(_emulate(x, wt, b, dtype, fault), ref, mag, dtype, name=fault)


def test_a_truncating_float32_store_is_below_what_any_float32_bound_can_see():
    """Why the fifth fault is planted on the 16-bit outputs only: truncating a float32 result moves it by less than one float32 ulp, 2 u32 |y| <= 2 u32 M."""
    x, wt, b = _operands("positive", F32)
    ref, mag = head64.pool_head_fwd64(x, wt, b)
    assert assert_fwd_close(_rtz(ref, F32), ref, mag, F32) <= 2.0


def test_global_pool_reference_and_magnitude():
    x = torch.randn(3, 16, 2, 5).to(BF16)
    ref, mag = head64.global_pool_fwd64(x)
    assert torch.equal(ref, x.double().mean((2, 3))) and torch.equal(mag, x.double().abs().mean((2, 3)))
    ref, mag = head64.pool_head_fwd64(x, torch.ones(1, 16), None)
    assert torch.allclose(ref[:, 0], x.double().mean((2, 3)).sum(1)) and bool((mag >= ref.abs()).all())
