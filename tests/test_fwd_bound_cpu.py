"""CPU: the per-element float64 bound of tests/fwd64.py, on models of the linear forward operators.

The float32 ATen chain stays inside the bound on the inputs of every case of tests/test_forward_f64_gpu.py, so a HIP kernel that misses it has no
excuse in the constant.  And on a float64 model of each operator (exact sums, one rounding at the store) five planted faults fall outside it, each
of which the bars it replaces (16-bit: |err| <= 1e-2 + 1e-2 |ref|; float32: max|err| < 1e-4) let through:

  a truncating 16-bit store; a float16 output rounded through bfloat16; one level's coarse plane held in the 16-bit type (RecConv2d);
  one border tap dropped on a pixel whose value is below 1e-3 of the plane maximum; a bias added twice on the last channel.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle.torch_eager import dwconv_eager, recconv2d_eager, upadd_dwconv_eager
from tests import fwd64
from tests import test_forward_f64_gpu as cases
from tests.fwd64 import K, assert_fwd_close, legacy_bar_holds
from tests.test_grad_bound_cpu import _rtz

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
SIXTEEN = [BF16, F16]


# ---- the float32 ATen chain on the GPU test's own inputs ---------------------------------------------------------------------------------------------------

def _worst(record_property, worst):
    record_property("worst_ratio", round(max(worst.values()), 3))
    print({k: round(v, 3) for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:5]})


@pytest.mark.parametrize("dts", list(cases.DT))
def test_float32_chain_is_inside_the_bound_recconv2d(dts, record_property):
    worst = {}
    for case in cases.RECCONV_CASES:
        if case[1] != dts:
            continue
        x, wd, wc, bd, bc = cases.recconv_inputs(case)
        ref, mag = fwd64.recconv2d_fwd64(x, wd, wc, bd, bc, case[2])
        got = recconv2d_eager(x, wd, wc, bd, bc, case[2]).to(cases.DT[dts])
        worst[cases.recconv_id(case)] = assert_fwd_close(got, ref, mag, cases.DT[dts], k=cases.CASE_K.get(cases.recconv_id(case)), name=cases.recconv_id(case))
        if case[4] == "positive":                             # nothing cancels, so the bound is a relative one however deep the ladder: M / |ref| is
            assert float((mag / ref.abs()).median()) < 3.0, cases.recconv_id(case)          # 1.2 .. 1.6 (2.1 on the 45 elements of 1 x 3 x 5 x 3)
    assert len(worst) == len(cases.RECCONV) * 8
    _worst(record_property, worst)


def test_float32_chain_is_inside_the_bound_dwconv2d(record_property):
    worst = {}
    for case in cases.DW_CASES:
        _, _, stride, (_, dout) = case
        x, w, b = cases.dw_inputs(case)
        for bias in (b, None):
            ref, mag = fwd64.dwconv_fwd64(x, w, bias, stride)
            worst[(cases.dw_id(case), bias is None)] = assert_fwd_close(dwconv_eager(x, w, bias, stride).to(dout), ref, mag, dout, name=cases.dw_id(case))
    _worst(record_property, worst)


def test_float32_chain_is_inside_the_bound_dwconv2d_mult2(record_property):
    worst = {}
    for case in cases.MULT2_CASES:
        _, _, k, stride, dts = case
        x, w, b = cases.mult2_inputs(case)
        for bias in (b, None):
            ref, mag = fwd64.dwconv_mult2_fwd64(x, w, bias, stride)
            got = F.conv2d(x, w, bias, stride=stride, padding=k // 2, groups=x.shape[1]).to(cases.DT[dts])
            worst[(cases.mult2_id(case), bias is None)] = assert_fwd_close(got, ref, mag, cases.DT[dts], name=cases.mult2_id(case))
    _worst(record_property, worst)


def test_float32_chain_is_inside_the_bound_upadd_dwconv(record_property):
    worst = {}
    for case in cases.UP_CASES:
        _, (_, _, odt), mode = case
        x, cs, w, b = cases.up_inputs(case)
        for bias in (b, None):
            ref, mag = fwd64.upadd_dwconv_fwd64(x, cs, w, bias, mode)
            got = (dwconv_eager(x, w, bias) if cs is None else upadd_dwconv_eager(x, cs, w, bias, mode)).to(odt)
            worst[(cases.up_id(case), bias is None)] = assert_fwd_close(got, ref, mag, odt, name=cases.up_id(case))
    _worst(record_property, worst)


def test_float32_chain_is_inside_the_bound_grouped_conv2d(record_property):
    worst = {}
    for case in cases.GROUPED_CASES:
        (_, _, _, _, _, groups), dts = case
        x, w, b = cases.grouped_inputs(case)
        for bias in (b, None):
            ref, mag = fwd64.grouped_conv2d_fwd64(x, w, bias, groups)
            got = F.conv2d(x, w, bias, stride=2, padding=2, groups=groups).to(cases.DT[dts])
            worst[(cases.grouped_id(case), bias is None)] = assert_fwd_close(got, ref, mag, cases.DT[dts], name=cases.grouped_id(case))
    _worst(record_property, worst)


# ---- float64 models with a place for each fault -------------------------------------------------------------------------------------------------------------

def _rand(g, shape, dtype=F32, scale=1.0):
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype).to(torch.float64)


def _ladder(x, wd, wc, bd, bc, mode, coarse_hook=None):
    """recconv2d_eager, statement for statement, with a hook on each level's coarse plane (the conv's output before it is resized) -> (y, the
    final conv's input)."""
    c, k, level = x.shape[1], wd.shape[-1], len(wc) - 1
    pyramid = [x]
    while len(pyramid) <= level:
        pyramid.append(F.conv2d(pyramid[-1], wd, bd, stride=2, padding=k // 2, groups=c))
    carry = None
    for j in range(level):
        fine, coarse = pyramid[level - j - 1], pyramid[level - j]
        t = coarse if carry is None else coarse + carry
        t = F.conv2d(t, wc[j], None if bc is None else bc[j], padding=k // 2, groups=c)
        if coarse_hook is not None:
            t = coarse_hook(j, t)
        carry = F.interpolate(t, size=fine.shape[2:], mode=mode)
    t = x if carry is None else x + carry
    return F.conv2d(t, wc[level], None if bc is None else bc[level], padding=k // 2, groups=c), t


def _last_bias(dtype):
    """The last channel's bias of the models: adding it twice stays under the old bars (1e-4 for float32, 1e-2 for the 16-bit types) ..."""
    return 2.0 ** -14 if dtype == F32 else 2.0 ** -7


class Model:
    """One operator on one set of inputs: ref / mag by tests/fwd64.py, y = the exact float64 output, and what the faults need."""

    def __init__(self, name, dtype, band=False):
        self.name, self.dtype = name, dtype
        g = torch.Generator().manual_seed(sum(map(ord, name)) + 7 * DTYPES.index(dtype) + 1000 * band)
        self.hook = None                                      # RecConv2d only: (level, type) of the coarse plane held in 16 bits
        quiet = (lambda t, rows: t[:, :, :rows].mul_(2.0 ** -13)) if band else (lambda t, rows: t)
        bias = not band                                       # the band's border pixels are small only without a bias
        if name == "recconv2d":
            # 2 x 8 x 14 x 14, level 2; the band: 32 rows of which the first 23 are quiet, so that the first rows of every level of the ladder are
            n, c, h, w, k, self.level, self.mode = (1, 8, 32, 14, 5, 2, "bilinear") if band else (2, 8, 14, 14, 5, 2, "bilinear")
            self.x = _rand(g, (n, c, h, w), dtype)
            quiet(self.x, 23)
            self.w = [_rand(g, (c, 1, k, k), F32, 0.2) for _ in range(self.level + 2)]
            self.b = [_rand(g, (c,), F32, 0.1) for _ in range(self.level + 2)] if bias else None
            self.last_w, self.stride, self.mult = self.w[-1], 1, 1
        else:
            k, self.stride, self.mult, groups, self.mode = {"dwconv2d": (5, 2, 1, None, None), "dwconv2d_mult2": (7, 2, 2, None, None),
                                                            "upadd_dwconv": (5, 1, 1, None, "bilinear"), "grouped_conv2d": (5, 2, None, 4, None)}[name]
            n, c, h, w = (2, 8, 9, 13) if name == "grouped_conv2d" else (2, 8, 14, 14)
            cout = 12 if name == "grouped_conv2d" else c * self.mult
            self.groups = groups or c
            self.x = _rand(g, (n, c, h, w), dtype)
            quiet(self.x, k)
            self.coarse = _rand(g, (n, c, 7, 7), F32) if name == "upadd_dwconv" else None
            if self.coarse is not None:
                quiet(self.coarse, k)
            self.w = _rand(g, (cout, c // self.groups, k, k), F32, 0.2)
            self.b = [_rand(g, (cout,), F32, 0.1)] if bias else None
            self.last_w = self.w
        if bias:
            self.b[-1][-1] = _last_bias(dtype)
        self.ref, self.mag = self._fwd64()
        self.y, self.t = self.run()
        assert torch.equal(self.y, self.ref)                  # the model is the reference, statement for statement

    def _fwd64(self):
        b = self.b
        if self.name == "recconv2d":
            return fwd64.recconv2d_fwd64(self.x, self.w[0], self.w[1:], b and b[0], b and b[1:], self.mode)
        if self.name == "dwconv2d":
            return fwd64.dwconv_fwd64(self.x, self.w, b and b[0], self.stride)
        if self.name == "dwconv2d_mult2":
            return fwd64.dwconv_mult2_fwd64(self.x, self.w, b and b[0], self.stride)
        if self.name == "upadd_dwconv":
            return fwd64.upadd_dwconv_fwd64(self.x, self.coarse, self.w, b and b[0], self.mode)
        return fwd64.grouped_conv2d_fwd64(self.x, self.w, b and b[0], self.groups)

    def run(self, coarse_hook=None):
        """-> (exact output, the last conv's input)."""
        b = self.b
        if self.name == "recconv2d":
            return _ladder(self.x, self.w[0], self.w[1:], b and b[0], b and b[1:], self.mode, coarse_hook)
        t = self.x if self.coarse is None else self.x + F.interpolate(self.coarse, size=self.x.shape[2:], mode=self.mode)
        k = self.w.shape[-1]
        return F.conv2d(t, self.w, b and b[0], stride=self.stride, padding=k // 2, groups=self.groups), t

    def store(self, y):
        """float32 sums, each output rounded once, to nearest."""
        return y.to(F32).to(self.dtype)


OPERATORS = ["recconv2d", "dwconv2d", "dwconv2d_mult2", "upadd_dwconv", "grouped_conv2d"]
_MODELS = {}


def model(name, dtype, band=False):
    if (name, dtype, band) not in _MODELS:
        _MODELS[(name, dtype, band)] = Model(name, dtype, band)
    return _MODELS[(name, dtype, band)]


def _caught_only_by_the_new_bound(m, got):
    """The fault is outside the per-element bound, and inside the bar it replaces."""
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_fwd_close(got, m.ref, m.mag, m.dtype, name=m.name)
    assert legacy_bar_holds(got, m.ref, m.dtype), "the planted fault is too coarse: the old bar sees it as well"


@pytest.mark.parametrize("band", [False, True], ids=["plain", "quiet-border"])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", OPERATORS)
def test_the_fault_free_model_passes(name, dtype, band):
    m = model(name, dtype, band)
    assert assert_fwd_close(m.store(m.y), m.ref, m.mag, dtype, name=name) <= 1.0          # float32's own rounding of the exact sum: at most one u32 |ref| <= u32 M
    assert legacy_bar_holds(m.store(m.y), m.ref, dtype)


@pytest.mark.parametrize("dtype", SIXTEEN, ids=str)
@pytest.mark.parametrize("name", OPERATORS)
def test_truncating_store_is_caught(name, dtype):
    m = model(name, dtype)
    _caught_only_by_the_new_bound(m, _rtz(m.y.to(F32).double(), dtype))


@pytest.mark.parametrize("name", OPERATORS)
def test_float16_output_through_bfloat16_is_caught(name):
    m = model(name, F16)
    _caught_only_by_the_new_bound(m, m.y.to(F32).to(BF16).to(F16))


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("dtype", SIXTEEN, ids=str)
def test_coarse_plane_held_in_16_bits_is_caught(dtype, level):
    m = model("recconv2d", dtype)
    y, _ = m.run(coarse_hook=lambda j, t: t.to(F32).to(dtype).double() if j == level else t)
    _caught_only_by_the_new_bound(m, m.store(y))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", OPERATORS)
def test_dropped_border_tap_on_a_small_pixel_is_caught(name, dtype):
    """Output pixel (0, 0) of the last channel loses the tap that reads its row's third element: input pixel (0, k - 1 - k // 2) times weight
    (k // 2, k - 1).  The model's first rows are quiet (2**-13 of the rest), so that pixel is small and so is the product."""
    m = model(name, dtype, band=True)
    k = m.last_w.shape[-1]
    co = m.ref.shape[1] - 1
    ci = co // m.mult if m.name != "grouped_conv2d" else (co // (m.ref.shape[1] // m.groups)) * m.last_w.shape[1]          # the group's first input channel
    assert float(m.ref[0, co, 0, 0].abs()) < 1e-3 * float(m.ref.abs().max())
    tap = m.last_w[co, 0, k // 2, k - 1] * m.t[0, ci, 0, k - 1 - k // 2]
    assert tap != 0
    y = m.y.clone()
    y[0, co, 0, 0] -= tap
    with pytest.raises(AssertionError, match=rf"worst at \(n=0, c={co}, h=0, w=0\)"):
        assert_fwd_close(m.store(y), m.ref, m.mag, dtype, name=name)
    _caught_only_by_the_new_bound(m, m.store(y))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("name", OPERATORS)
def test_bias_added_twice_on_the_last_channel_is_caught(name, dtype):
    m = model(name, dtype)
    y = m.y.clone()
    y[:, -1] += m.b[-1][-1]
    assert float(m.b[-1][-1]) == _last_bias(dtype)
    _caught_only_by_the_new_bound(m, m.store(y))


@pytest.mark.parametrize("values", cases.VALUES)
def test_a_deep_ladder_is_held_by_values_that_do_not_cancel(values):
    """Level 4 on 56 x 56 in float32, the coarsest level's plane held in float16 (2**-12 of it lost).  On zero-mean values M is some 4e4 |ref|, the
    bound is percent of the output and the fault slips through; on the non-cancelling values of the GPU test's second set it is outside the bound."""
    case = ((1, 48, 56, 56, 4, 5), "f32", "bilinear", False, values)
    assert case in cases.RECCONV_CASES
    x, wd, wc, _, _ = cases.recconv_inputs(case)
    ref, mag = fwd64.recconv2d_fwd64(x, wd, wc, None, None, "bilinear")
    y, _ = _ladder(x.double(), wd.double(), [t.double() for t in wc], None, None, "bilinear", coarse_hook=lambda j, t: t.to(F32).to(F16).double() if j == 0 else t)
    assert_fwd_close(_ladder(x.double(), wd.double(), [t.double() for t in wc], None, None, "bilinear")[0].to(F32), ref, mag, F32)
    if values == "zero-mean":
        assert float((mag / ref.abs()).median()) > 1e4
        assert_fwd_close(y.to(F32), ref, mag, F32)
    else:
        with pytest.raises(AssertionError, match="outside the bound"):
            assert_fwd_close(y.to(F32), ref, mag, F32)


def test_the_constant_is_the_backward_one():
    from tests import grad64
    assert fwd64.K is grad64.K and K == 24.0 and fwd64.assert_fwd_close is grad64.assert_grad_close
