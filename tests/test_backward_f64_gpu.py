"""GPU: every backward schedule of RecConv2d, and the depthwise backward pieces of RecAttn2d / Downsample on both sides of their batch cut-overs,
against float64 autograd through the ATen restatement, element by element (tests/grad64.py: half a 16-bit ulp where the output is 16-bit, plus
K * 2**-24 times the sum of absolute products that feed the element).

Schedules of rcx_recconv2d_bwd (rcx_api.hip): "one7" / "one14" the one-launch block backward (N <= 512; at 14 x 14 two waves per plane while
2 * planes <= 1024 and planes % 8 == 0, planes = N * ceil(C / 64)), "tiled28" / "tiled56" the tiled adjoint kernels of the fine levels with the
one-launch 14 x 14 block as their tail, "perstep" one launch per ladder step, "generic" the same under RCX_FORCE_GENERIC=1.  Each case checks
that the library still routes it as named, through the plan query (rcx_recconv2d_bwd_plan) and through the dL/dy type it accepts (bfloat16 on
the first four, float32 on the last two).
"""
import itertools

import pytest
import torch

import recnext_amd
from recnext_amd import _lib, ops
from tests import grad64
from tests.grad64 import assert_grad_close, to_kkc

pytestmark = pytest.mark.gpu

K5 = 5
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# schedule, (N, C, H, W, level)
SMALL = [
    ("one7", (2, 512, 7, 7, 1)), ("one7", (3, 40, 7, 7, 1)),
    ("one14split", (2, 256, 14, 14, 2)), ("one14", (3, 100, 14, 14, 2)),
    ("tiled28", (2, 128, 28, 28, 3)), ("tiled28", (1, 96, 28, 28, 3)),
    ("tiled56", (2, 64, 56, 56, 4)), ("tiled56", (1, 4, 56, 56, 4)), ("tiled56", (2, 68, 56, 56, 4)),
    ("perstep", (1, 8, 25, 13, 2)), ("perstep", (2, 12, 9, 9, 0)), ("perstep", (1, 12, 15, 22, 2)), ("perstep", (1, 8, 40, 40, 5)),
    ("perstep", (1, 16, 64, 64, 3)),
    ("generic", (2, 64, 56, 56, 4)), ("generic", (2, 256, 14, 14, 2)),
]
# the training-batch sizes on both sides of each cut: bfloat16 with native dL/dy and bias, the mode alternating, and one float32 case per schedule
LARGE = [
    ("one7", (512, 8, 7, 7, 1), "bf16", "bilinear"), ("perstep", (513, 8, 7, 7, 1), "bf16", "nearest"),
    ("one14split", (128, 256, 14, 14, 2), "bf16", "nearest"), ("one14", (130, 256, 14, 14, 2), "bf16", "bilinear"),
    ("tiled28", (128, 128, 28, 28, 3), "bf16", "bilinear"), ("tiled28", (288, 128, 28, 28, 3), "bf16", "nearest"),
    ("tiled56", (64, 64, 56, 56, 4), "bf16", "nearest"), ("tiled56", (160, 64, 56, 56, 4), "bf16", "bilinear"),
    ("one7", (512, 8, 7, 7, 1), "f32", "nearest"), ("perstep", (513, 8, 7, 7, 1), "f32", "bilinear"),
    ("one14split", (128, 256, 14, 14, 2), "f32", "bilinear"), ("tiled28", (288, 128, 28, 28, 3), "f32", "bilinear"),
    ("tiled56", (160, 64, 56, 56, 4), "f32", "nearest"),
]
FAST = ("one7", "one14split", "one14", "tiled28", "tiled56")


def _plan(sched, n, c):
    """The plan string of each schedule; the tiled ones end in their 14 x 14 tail, split by the rule above."""
    planes = n * -(-c // 64)
    tail = "one(k_recconv_bwd_cpl14,split)" if 2 * planes <= 1024 and planes % 8 == 0 else "one(k_recconv_bwd_cpl14)"
    return {"one7": "one(k_recconv_bwd_cpl7)", "one14": "one(k_recconv_bwd_cpl14)", "one14split": "one(k_recconv_bwd_cpl14,split)",
            "tiled28": "tiled(levels=1)+" + tail, "tiled56": "tiled(levels=2)+" + tail, "perstep": "steps", "generic": "generic"}[sched]


RECCONV_CASES = [(s, shp, dt, mode, bias) for (s, shp), dt, mode, bias in
                 itertools.product(SMALL, ("f32", "bf16", "f16"), ("bilinear", "nearest"), (True, False))]
RECCONV_CASES += [(s, shp, dt, mode, True) for s, shp, dt, mode in LARGE]


def _id(case):
    s, (n, c, h, w, level), dt, mode, bias = case
    return f"{s}-{n}x{c}x{h}x{w}L{level}-{dt}-{mode}-{'bias' if bias else 'nobias'}"


def _rand(g, shape, dtype, dev, scale=1.0):
    """Normal values rounded to dtype, held in float32 (exactly representable in dtype)."""
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype).to(torch.float32).to(dev)


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


@pytest.fixture
def ratios(record_property):
    """Records every output's worst err / (u32 * M) as a test property (in the junit report), to keep K honest."""
    seen = {}

    def add(name, r):
        seen[name] = r
    yield add
    if seen:
        record_property("worst_ratio", max(seen.values()))
        record_property("ratios", {k: round(v, 3) for k, v in seen.items()})


@pytest.mark.parametrize("case", RECCONV_CASES, ids=_id)
def test_recconv2d_backward_matches_float64(case, monkeypatch, ratios):
    sched, (n, c, h, w, level), dts, mode, bias = case
    if sched == "generic":
        monkeypatch.setenv("RCX_FORCE_GENERIC", "1")
    dt = DT[dts]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(n * 7919 + c * 131 + h * 17 + level + 3 * (mode == "nearest") + 5 * bias)
    x32 = _rand(g, (n, c, h, w), dt, dev)
    gy32 = _rand(g, (n, c, h, w), dt, dev)
    wd = _rand(g, (c, 1, K5, K5), dt, dev, 0.2)
    wc = [_rand(g, (c, 1, K5, K5), dt, dev, 0.2) for _ in range(level + 1)]
    bd = _rand(g, (c,), dt, dev, 0.1) if bias else None
    bc = [_rand(g, (c,), dt, dev, 0.1) for _ in range(level + 1)] if bias else None

    assert ops.recconv2d_bwd_plan(n, c, h, w, level, K5, dt) == _plan(sched, n, c)
    gy_native = _lib.load().rcx_recconv2d_bwd_gy_dtype(n, c, h, w, level, K5, ops._DT[dt])
    if dt == torch.bfloat16:
        assert gy_native == (_lib.DTYPE_BF16 if sched in FAST else _lib.DTYPE_F32), "the case no longer reaches the schedule it is named after"
    if sched in ("perstep", "generic"):
        assert _lib.load().rcx_recconv2d_bwd_gy_dtype(n, c, h, w, level, K5, _lib.DTYPE_BF16) == _lib.DTYPE_F32

    ref, mag = grad64.recconv2d_grads64(x32, gy32, wd, wc, bd, bc, mode)
    names = ["down"] + [f"convs.{i}" for i in range(level + 1)]

    # the C entry through ops: packed float32 parameter gradients; dL/dy in float32, and (bfloat16) as it is where the library reads it natively
    x = _cl(x32.to(dt))
    wpack, bpack = ops.pack_recconv_params(wd, wc, bd, bc)
    _, saved = ops.recconv2d_forward_train(x, wpack, bpack, level, K5, mode)
    gys = [("gy32", _cl(gy32))]
    if gy_native == _lib.DTYPE_BF16:
        gys.append(("gybf16", _cl(gy32.to(dt))))
    for tag, gy in gys:
        gx, gw, gb = ops.recconv2d_backward(x, gy, wpack, saved, level, K5, mode, need_bias=bias)
        assert gx.dtype == dt
        ratios(f"ops/{tag}/gx", assert_grad_close(gx, ref["gx"], mag["gx"], dt, name=f"ops/{tag} gx"))
        for i, nm in enumerate(names):
            ratios(f"ops/{tag}/{nm}.weight", assert_grad_close(gw[i], to_kkc(ref["gw"][i]), to_kkc(mag["gw"][i]), torch.float32,
                                                             name=f"ops/{tag} {nm}.weight", layout="kkc"))
            if bias:
                ratios(f"ops/{tag}/{nm}.bias", assert_grad_close(gb[i], ref["gb"][i], mag["gb"][i], torch.float32, name=f"ops/{tag} {nm}.bias", layout="c"))

    # the module's autograd path: parameters in x's dtype, their gradients written in that dtype by the backward's final reduction
    mod = recnext_amd.RecConv2d(c, K5, bias, level, mode)
    sd = {"down.weight": wd, **{f"convs.{i}.weight": t for i, t in enumerate(wc)}}
    if bias:
        sd.update({"down.bias": bd, **{f"convs.{i}.bias": t for i, t in enumerate(bc)}})
    mod.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    mod = mod.to(device=dev, dtype=dt).train()
    xm = x.clone().requires_grad_(True)
    params = list(mod.parameters())
    grads = torch.autograd.grad(mod(xm), [xm] + params, _cl(gy32.to(dt)))
    ratios("module/gx", assert_grad_close(grads[0], ref["gx"], mag["gx"], dt, name="module gx"))
    it = iter(grads[1:])
    for i, nm in enumerate(names):
        gwi = next(it)
        assert gwi.dtype == dt and gwi.shape == (c, 1, K5, K5)
        ratios(f"module/{nm}.weight", assert_grad_close(gwi, ref["gw"][i], mag["gw"][i], dt, name=f"module {nm}.weight", layout="ckk"))
        if bias:
            ratios(f"module/{nm}.bias", assert_grad_close(next(it), ref["gb"][i], mag["gb"][i], dt, name=f"module {nm}.bias", layout="c"))


# ---- depthwise backward pieces at their batch cut-overs (N * H / 14 <= 512 partial rows: tiled weight gradient, above: the generic reduction) ----

def _check_dw(ratios, tag, dt, gx, gw, gb, ref, mag):
    if gx is not None:
        assert gx.dtype == dt
        ratios(f"{tag}/gx", assert_grad_close(gx, ref[0], mag[0], dt, name=f"{tag} gx"))
    ratios(f"{tag}/gw", assert_grad_close(gw, to_kkc(ref[1]), to_kkc(mag[1]), torch.float32, name=f"{tag} gw", layout="kkc"))
    ratios(f"{tag}/gb", assert_grad_close(gb, ref[2], mag[2], torch.float32, name=f"{tag} gb", layout="c"))


@pytest.mark.parametrize("dts", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n,c,h", [(128, 64, 56), (129, 64, 56), (256, 32, 28), (257, 32, 28)], ids=lambda v: str(v))
def test_dwconv2d_stride2_backward_matches_float64(n, c, h, dts, ratios):
    dt, dev = DT[dts], torch.device("cuda:0")
    g = torch.Generator().manual_seed(n + c + h)
    x32 = _rand(g, (n, c, h, h), dt, dev)
    gy = _rand(g, (n, c, h // 2, h // 2), dt, dev)
    w = _rand(g, (c, 1, K5, K5), dt, dev, 0.2)
    b = _rand(g, (c,), dt, dev, 0.1)
    ref, mag = grad64.dwconv_grads64(x32, gy, w, b, stride=2)
    gx, gw, gb = ops.dwconv2d_backward(_cl(x32.to(dt)), _cl(gy), to_kkc(w).contiguous(), K5, 2, need_bias=True)
    _check_dw(ratios, "dwconv2d", dt, gx, gw, gb, ref, mag)


@pytest.mark.parametrize("mode", ["nearest", "bilinear"])
@pytest.mark.parametrize("dts", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n", [2, 160])
def test_upadd_dwconv_backward_matches_float64(n, dts, mode, ratios):
    c, h, dt, dev = 64, 56, DT[dts], torch.device("cuda:0")
    g = torch.Generator().manual_seed(n + 3 * (mode == "nearest"))
    x32 = _rand(g, (n, c, h, h), dt, dev)
    coarse = _rand(g, (n, c, h // 2, h // 2), torch.float32, dev)
    gy32 = _rand(g, (n, c, h, h), dt, dev)
    w = _rand(g, (c, 1, K5, K5), dt, dev, 0.2)
    b = _rand(g, (c,), dt, dev, 0.1)
    ref, mag = grad64.upadd_dwconv_grads64(x32, coarse, gy32, w, b, mode)
    native = _lib.load().rcx_upadd_dwconv_bwd_gy_dtype(n, c, h, h, h // 2, h // 2, K5, ops._DT[dt])
    assert native == (_lib.DTYPE_BF16 if dt == torch.bfloat16 else _lib.DTYPE_F32)
    gys = [("gy32", gy32)] + ([("gybf16", gy32.to(dt))] if native == _lib.DTYPE_BF16 else [])
    x = _cl(x32.to(dt))
    for tag, gy in gys:
        gx, gc, gw, gb = ops.upadd_dwconv_backward(x, _cl(coarse), _cl(gy), to_kkc(w).contiguous(), K5, mode, need_bias=True)
        ratios(f"{tag}/gcoarse", assert_grad_close(gc, ref[1], mag[1], torch.float32, name=f"upadd/{tag} gcoarse"))
        _check_dw(ratios, f"upadd/{tag}", dt, gx, gw, gb, (ref[0], ref[2], ref[3]), (mag[0], mag[2], mag[3]))


@pytest.mark.parametrize("dts", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n,c,h", [(128, 32, 56), (129, 32, 56), (2, 104, 14)], ids=lambda v: str(v))
def test_dwconv2d_mult2_backward_matches_float64(n, c, h, dts, ratios):
    k, dt, dev = 7, DT[dts], torch.device("cuda:0")
    g = torch.Generator().manual_seed(n * 3 + c + h)
    x32 = _rand(g, (n, c, h, h), dt, dev)
    gy = _rand(g, (n, 2 * c, h // 2, h // 2), dt, dev)
    w = _rand(g, (2 * c, 1, k, k), dt, dev, 0.15)
    b = _rand(g, (2 * c,), dt, dev, 0.1)
    ref, mag = grad64.dwconv_mult2_grads64(x32, gy, w, b)
    gx, gw, gb = ops.dwconv2d_mult2_backward(_cl(x32.to(dt)), _cl(gy), to_kkc(w).contiguous(), k, need_bias=True)
    _check_dw(ratios, "mult2", dt, gx, gw, gb, ref, mag)
