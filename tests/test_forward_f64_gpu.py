"""GPU: every linear forward kernel against float64, element by element (tests/fwd64.py: half a 16-bit ulp where the output is 16-bit, plus
K * 2**-24 times the sum of the absolute products that feed the element; K = grad64.K), in float32, bfloat16 and float16, both resize modes, with
and without bias.

  ops.recconv2d_forward        at the extents of tests/test_guard_bands_gpu.py (RECCONV: the smallest that select each of the eleven forward
                               schedule families, asserted below), and every extent again on the generic ladder (RCX_FORCE_GENERIC=1); each
                               with zero-mean values and with values that do not cancel (VALUES below: on a deep ladder only those keep the
                               bound at two parts in a million of the output)
  ops.recconv2d_forward_train  its y, on the same cases where C % 4 == 0
  ops.dwconv2d                 k 3 / 5 / 7, stride 1 / 2, the guard table's type pairs and planes
  ops.dwconv2d_mult2           the lanes kernel (28 x 28), the tiled one (14 x 14; float16; a plane the lanes kernel has no plan for), the generic one
  ops.upadd_dwconv             an extent for every answer of upadd_dwconv_plan, the guard table's (x, coarse, out) type triples, coarse=None
  ops.grouped_conv2d           SHAPES of tests/test_ls_down_gpu.py

The inputs of a case are made on the CPU by the *_inputs functions below (tests/test_fwd_bound_cpu.py holds the float32 ATen chain to the same
bound on the same inputs); the references are computed once a case.  A test runs every combination of one extent (the *_CASES lists hold them one
by one; the test reports all that fail, each by its own id) and records its worst err / (2**-24 * M), whole and per kernel and output type, as
properties: 131 tests over 863 cases, so that the suite's report grows by a line an extent.
"""
import itertools
import zlib

import pytest
import torch

from recnext_amd import ops
from tests import fwd64
from tests.fwd64 import assert_fwd_close
from tests.test_guard_bands_gpu import FWD_FAMILIES, MODES, RECCONV, STEP_PLANES, plan_family
from tests.test_ls_down_gpu import SHAPES as GROUPED_SHAPES
from tests.util import rcx_env

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT = {"f32": F32, "bf16": BF16, "f16": F16}
DT_ID = {v: k for k, v in DT.items()}

# A case whose float32 ATen chain itself exceeds K on the CPU (a deep ladder) carries its own K here, by its id: four times the chain's ratio, with
# the chain's figure beside it.  None does: over the cases of this file the chain's worst ratio is 6.2 on the ladders (level 5: 5.6) and 5.6 on
# the single convs (tests/test_fwd_bound_cpu.py prints them).
CASE_K = {}


def gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()))


def rnd(g, shape, dtype=F32, scale=1.0):
    """Normal values rounded to dtype, held in float32 on the CPU (exactly representable in dtype)."""
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype).to(torch.float32)


def dev(t, dtype=None):
    """A CPU tensor on the GPU in dtype; four-dimensional ones channels_last."""
    if t is None:
        return None
    t = t.to("cuda:0")
    if dtype is not None:
        t = t.to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


class Held:
    """Checks outputs against the bound, remembers every worst ratio and every failure, and fails the test at the end with all of them."""

    def __init__(self, record_property):
        self.record, self.seen, self.failed = record_property, {}, []

    def __call__(self, kernel, where, got, ref, mag, out_dtype, k=None):
        """kernel: what ran (the row of the table); where: the case and variant, for the message.  Figures are kept per kernel and output type."""
        key, name = f"{kernel} {DT_ID[out_dtype]}", f"{kernel} [{where}]"
        ratio = assert_fwd_close(got, ref, mag, out_dtype, k=float("inf"), name=name)        # the figure, whatever it is
        worst, n = self.seen.get(key, (0.0, 0))
        self.seen[key] = (max(worst, ratio), n + 1)
        try:
            assert_fwd_close(got, ref, mag, out_dtype, k=k, name=name)
        except AssertionError as e:
            self.failed.append(str(e))

    def finish(self):
        assert self.seen
        ratios = {key: (round(worst, 2), n) for key, (worst, n) in self.seen.items()}          # key -> (worst ratio, checks)
        self.record("worst_ratio", max(r for r, _ in ratios.values()))
        self.record("ratios", ratios)
        print("ratios:", ratios)
        assert not self.failed, "\n".join(self.failed)


@pytest.fixture
def held(record_property):
    return Held(record_property)


# ---- RecConv2d -------------------------------------------------------------------------------------------------------------------------------------------

# Two sets of values for every case.  "zero-mean": x ~ N(0, 1), w ~ 0.2 N(0, 1), as the guard table and the backward's tests draw them.  With
# zero-mean weights a conv's sum of |w| is four to five times the size of what it adds up to, and a ladder multiplies that factor at every conv:
# M / |ref| (median over a plane) is about 4 on a single conv, 300 at level 2, 5e4 at level 4 and 5e5 at level 5, so on a deep ladder K * 2**-24 * M
# is some percent of the output and only the half-ulp term of a 16-bit output stays sharp.  "positive": x ~ 1 + N(0, 1), w ~ (1 + N(0, 1) / 2) / k**2
# (a smoothing kernel of unit sum, one tap in fifty negative, as a trained RecConv2d's low-pass levels are): nothing cancels on the way up, M / |ref|
# is 1.5 at every level (tests/test_fwd_bound_cpu.py asserts it) and the bound is 24 * 2**-24 * 1.5 |ref|, two parts in a million, at level 5 as at
# level 0.  The first keeps the signs and the cancellation honest, the second keeps the bound tight where the ladder is deep.
VALUES = ("zero-mean", "positive")
RECCONV_CASES = list(itertools.product(RECCONV, DT, MODES, (True, False), VALUES))


def recconv_id(case):
    ext, dts, mode, bias, values = case
    return f"{'x'.join(map(str, ext))}-{dts}-{mode}-{'bias' if bias else 'nobias'}-{values}"


def recconv_inputs(case):
    """-> x (in the I/O type's values), w_down, w_convs, b_down | None, b_convs | None: float32 on the CPU."""
    (n, c, h, w, level, k), dts, mode, bias, values = case
    g = gen("recconv", case)
    if values == "positive":
        x = (1 + torch.randn((n, c, h, w), generator=g)).to(DT[dts]).to(F32)
        wd, *wc = [((1 + 0.5 * torch.randn((c, 1, k, k), generator=g)) / (k * k)).to(F32) for _ in range(level + 2)]
    else:
        x = rnd(g, (n, c, h, w), DT[dts])
        wd, *wc = [rnd(g, (c, 1, k, k), F32, 0.2) for _ in range(level + 2)]
    bd = rnd(g, (c,), F32, 0.1) if bias else None
    bc = [rnd(g, (c,), F32, 0.1) for _ in range(level + 1)] if bias else None
    return x, wd, wc, bd, bc


def test_the_cases_reach_every_forward_family():
    hit = {plan_family(ops.recconv2d_plan(*ext, mode, DT[dts])) for ext, dts, mode, _, _ in RECCONV_CASES}
    assert hit == FWD_FAMILIES, (sorted(FWD_FAMILIES - hit), sorted(hit - FWD_FAMILIES))
    assert len(FWD_FAMILIES) == 11


def gathered(cases, key):
    """The cases in their order, gathered by key(case): one test runs a group, so that the report holds a line per extent and not per combination."""
    groups = {}
    for case in cases:
        groups.setdefault(key(case), []).append(case)
    return list(groups.items())


def group_id(group):
    return group[0]


def recconv_case(case, held):
    (n, c, h, w, level, k), dts, mode, bias, _ = case
    dt, cid = DT[dts], recconv_id(case)
    x32, wd, wc, bd, bc = recconv_inputs(case)
    ref, mag = fwd64.recconv2d_fwd64(x32, wd, wc, bd, bc, mode)
    kk = CASE_K.get(cid)

    x = dev(x32, dt)
    wpack, bpack = ops.pack_recconv_params(dev(wd), [dev(t) for t in wc], dev(bd), [dev(t) for t in bc] if bias else None)
    fam = plan_family(ops.recconv2d_plan(n, c, h, w, level, k, mode, dt))
    y = ops.recconv2d_forward(x, wpack, bpack, level, k, mode)
    assert y.dtype == dt and y.shape == x.shape
    held(f"forward/{fam}", cid, y, ref, mag, dt, kk)
    if c % 4 == 0:
        yt, _ = ops.recconv2d_forward_train(x, wpack, bpack, level, k, mode)
        assert yt.dtype == dt
        held("train/y", cid, yt, ref, mag, dt, kk)
    with rcx_env(RCX_FORCE_GENERIC="1"):
        assert plan_family(ops.recconv2d_plan(n, c, h, w, level, k, mode, dt)) == "generic"
        yg = ops.recconv2d_forward(x, wpack, bpack, level, k, mode)
        torch.cuda.synchronize()
    held("forward/forced-generic", cid, yg, ref, mag, dt, kk)


# one test an extent and I/O type: both resize modes, with and without bias, both sets of values
@pytest.mark.parametrize("group", gathered(RECCONV_CASES, lambda case: f"{'x'.join(map(str, case[0]))}-{case[1]}"), ids=group_id)
def test_recconv2d_forward_matches_float64(group, held):
    assert len(group[1]) == len(MODES) * 2 * len(VALUES)
    for case in group[1]:
        recconv_case(case, held)
    held.finish()


# ---- the depthwise conv ------------------------------------------------------------------------------------------------------------------------------------

DW_PAIRS = [(F32, F32), (BF16, F32), (BF16, BF16), (F32, BF16), (F16, F16)]          # (input, output) of the guard table
DW_PLANES = [(5, 3), (7, 7), (9, 11), (14, 14), (30, 44)]
assert sorted(DW_PLANES) == sorted(STEP_PLANES)
DW_CASES = list(itertools.product(DW_PLANES, (3, 5, 7), (1, 2), DW_PAIRS))


def dw_id(case):
    (h, w), k, stride, (din, dout) = case
    return f"{h}x{w}-k{k}s{stride}-{DT_ID[din]}-{DT_ID[dout]}"


def dw_inputs(case):
    """-> x (2, C, H, W), w (C,1,k,k), b (C): float32 on the CPU; C = 24 or 40 by the type pair, as the guard table has it."""
    (h, w), k, stride, (din, dout) = case
    c = 24 if DW_PAIRS.index((din, dout)) % 2 == 0 else 40
    g = gen("dwconv", dw_id(case))
    return rnd(g, (2, c, h, w), din), rnd(g, (c, 1, k, k), F32, 0.2), rnd(g, (c,), F32, 0.1)


def dw_case(case, held):
    _, k, stride, (din, dout) = case
    x32, w, b = dw_inputs(case)
    x, wk, bk = dev(x32, din), ops.pack_dw_weight(dev(w)), ops.pack_bias(dev(b))
    for bias in (True, False):
        ref, mag = fwd64.dwconv_fwd64(x32, w, b if bias else None, stride)
        where = f"{dw_id(case)}-{'bias' if bias else 'nobias'}"
        y = ops.dwconv2d(x, wk, bk if bias else None, k=k, stride=stride, out_dtype=dout)
        assert y.dtype == dout and tuple(y.shape) == tuple(ref.shape)
        held("as dispatched", where, y, ref, mag, dout)
        with rcx_env(RCX_FORCE_GENERIC="1"):
            yg = ops.dwconv2d(x, wk, bk if bias else None, k=k, stride=stride, out_dtype=dout)
            torch.cuda.synchronize()
        held("forced-generic", where, yg, ref, mag, dout)


# one test a plane, k and stride: every type pair, with and without bias
@pytest.mark.parametrize("group", gathered(DW_CASES, lambda case: dw_id(case).rsplit("-", 2)[0]), ids=group_id)
def test_dwconv2d_matches_float64(group, held):
    assert len(group[1]) == len(DW_PAIRS)
    for case in group[1]:
        dw_case(case, held)
    held.finish()


# ---- the channel-multiplier-2 conv of Downsample ---------------------------------------------------------------------------------------------------------------

# (kernel, (N, C, H, W), k, stride, types).  rcx_dwconv2d_mult2_fwd has no plan query; by its dispatch (rcx_api.hip) the register-resident lanes kernel
# takes k = 7, stride 2 on the 28 .. 64 squares in float32 / bfloat16 with C % 16 == 0 (four waves at C = 16, eight at 32), the tiled kernel every
# other even plane of at least 14 x 14 with k = 7, stride 2 (14 x 14; float16; 30 x 44), and the generic kernel the rest (odd planes, k != 7, stride 1).
MULT2 = [
    ("lanes", (2, 32, 28, 28), 7, 2, ("f32", "bf16")), ("lanes", (3, 16, 28, 28), 7, 2, ("f32", "bf16")),
    ("tiled", (2, 24, 14, 14), 7, 2, ("f32", "bf16", "f16")), ("tiled", (2, 32, 28, 28), 7, 2, ("f16",)), ("tiled", (1, 40, 30, 44), 7, 2, ("f32", "bf16", "f16")),
    ("generic", (2, 6, 9, 11), 7, 2, ("f32", "bf16", "f16")), ("generic", (2, 6, 9, 11), 5, 2, ("f32", "bf16", "f16")), ("generic", (2, 6, 5, 3), 3, 1, ("f32", "bf16", "f16")),
    ("generic", (2, 24, 14, 14), 7, 1, ("f32", "bf16", "f16")),
]
MULT2_CASES = [(kern, shape, k, stride, dts) for kern, shape, k, stride, types in MULT2 for dts in types]


def mult2_id(case):
    kern, shape, k, stride, dts = case
    return f"{kern}-{'x'.join(map(str, shape))}-k{k}s{stride}-{dts}"


def mult2_inputs(case):
    _, (n, c, h, w), k, _, dts = case
    g = gen("mult2", mult2_id(case))
    return rnd(g, (n, c, h, w), DT[dts]), rnd(g, (2 * c, 1, k, k), F32, 0.15), rnd(g, (2 * c,), F32, 0.1)


def mult2_case(case, held):
    kern, _, k, stride, dts = case
    dt = DT[dts]
    x32, w, b = mult2_inputs(case)
    x, wk, bk = dev(x32, dt), ops.pack_dw_weight(dev(w)), ops.pack_bias(dev(b))
    for bias in (True, False):
        ref, mag = fwd64.dwconv_mult2_fwd64(x32, w, b if bias else None, stride)
        where = f"{mult2_id(case)}-{'bias' if bias else 'nobias'}"
        y = ops.dwconv2d_mult2(x, wk, bk if bias else None, k=k, stride=stride)
        assert y.dtype == dt and tuple(y.shape) == tuple(ref.shape)
        held(kern, where, y, ref, mag, dt)
        if kern != "generic":
            with rcx_env(RCX_FORCE_GENERIC="1"):
                yg = ops.dwconv2d_mult2(x, wk, bk if bias else None, k=k, stride=stride)
                torch.cuda.synchronize()
            held(f"{kern}/forced-generic", where, yg, ref, mag, dt)


# one test a row of MULT2: its types, with and without bias
@pytest.mark.parametrize("group", gathered(MULT2_CASES, lambda case: mult2_id(case).rsplit("-", 1)[0]), ids=group_id)
def test_dwconv2d_mult2_matches_float64(group, held):
    for case in group[1]:
        mult2_case(case, held)
    held.finish()


# ---- conv_k(x + resize(coarse)) ----------------------------------------------------------------------------------------------------------------------------------

UP_TRIPLES = [(F32, F32, F32), (BF16, F32, F32), (BF16, BF16, BF16), (F32, BF16, F32), (F16, F32, F16), (F16, F16, F16)]          # (x, coarse, out) of the guard table
# (C, plane, coarse plane | None, k) -> the kernel upadd_dwconv_plan names where out has x's type (the lanes kernels have no float16 form: those go to
# what the last column names); an output of another type than x's is the generic kernel's everywhere.
UP_EXTENTS = [
    (64, (7, 7), (4, 4), 5, "cpl7", "cpl7"), (40, (14, 14), (7, 7), 5, "cpl14", "cpl14"),
    (64, (28, 28), (14, 14), 5, "cpt", "cpt"), (24, (30, 44), (15, 22), 5, "cpt", "cpt"),
    (48, (28, 28), (14, 14), 5, "lanes", "cpt"), (16, (32, 32), (16, 16), 5, "lanes", "cpt"),
    (16, (16, 16), (8, 8), 5, "generic", "generic"), (16, (9, 11), (5, 6), 5, "generic", "generic"), (16, (5, 3), (1, 1), 5, "generic", "generic"),
    (16, (14, 14), (7, 7), 3, "generic", "generic"), (16, (9, 11), (5, 6), 7, "generic", "generic"),
    (16, (14, 14), None, 5, "conv5_lanes", "generic"), (32, (28, 28), None, 5, "conv5_lanes", "generic"), (16, (9, 11), None, 5, "generic", "generic"),
    (16, (16, 16), None, 7, "generic", "generic"),
]
UP_KINDS = {"cpl7", "cpl14", "cpt", "lanes", "conv5_lanes", "generic"}
# without a coarse plane its type and the mode say nothing: one case for each (x, out) pair of the triples
UP_PAIRS = [tr for i, tr in enumerate(UP_TRIPLES) if (tr[0], tr[2]) not in {(u[0], u[2]) for u in UP_TRIPLES[:i]}]
UP_CASES = [(ext, tr, mode) for ext in UP_EXTENTS for tr in UP_TRIPLES for mode in MODES if ext[2] is not None or (tr in UP_PAIRS and mode == "nearest")]


def up_kind(plan):
    head = plan.split("(")[0]
    if head == "upadd_cpl14":
        return "cpl7" if "cpl7" in plan else "cpl14"
    return {"upadd_cpt": "cpt", "upadd_lanes": "lanes", "conv5_lanes": "conv5_lanes", "generic": "generic"}[head]


def up_expected(case):
    (c, plane, coarse, k, native, native16), (xdt, cdt, odt), mode = case
    if odt != xdt or cdt not in (xdt, F32):
        return "generic"
    return native16 if xdt == F16 else native


def up_plan(case):
    (c, (h, w), coarse, k, _, _), (xdt, cdt, odt), mode = case
    hc, wc = coarse if coarse is not None else (0, 0)
    return ops.upadd_dwconv_plan(2, c, h, w, hc, wc, k, mode, xdt, cdt if coarse is not None else None, odt)


def up_id(case):
    (c, (h, w), coarse, k, _, _), (xdt, cdt, odt), mode = case
    return f"{c}x{h}x{w}-{'x'.join(map(str, coarse)) if coarse else 'nocoarse'}-k{k}-{mode}-{DT_ID[xdt]}-{DT_ID[cdt]}-{DT_ID[odt]}"


def up_inputs(case):
    (c, (h, w), coarse, k, _, _), (xdt, cdt, odt), mode = case
    g = gen("upadd", up_id(case))
    return (rnd(g, (2, c, h, w), xdt), rnd(g, (2, c) + tuple(coarse), cdt) if coarse is not None else None, rnd(g, (c, 1, k, k), F32, 0.2), rnd(g, (c,), F32, 0.1))


def test_the_upadd_cases_reach_every_kernel():
    assert {up_kind(up_plan(case)) for case in UP_CASES} == UP_KINDS


def up_case(case, held):
    (c, (h, w), coarse, k, _, _), (xdt, cdt, odt), mode = case
    kind = up_kind(up_plan(case))
    assert kind == up_expected(case), f"{up_id(case)} no longer reaches the kernel it is there for"
    x32, cs32, wt, b = up_inputs(case)
    x, cs, wk, bk = dev(x32, xdt), dev(cs32, cdt), ops.pack_dw_weight(dev(wt)), ops.pack_bias(dev(b))
    for bias in (True, False):
        ref, mag = fwd64.upadd_dwconv_fwd64(x32, cs32, wt, b if bias else None, mode)
        where = f"{up_id(case)}-{'bias' if bias else 'nobias'}"
        y = ops.upadd_dwconv(x, cs, wk, bk if bias else None, k=k, mode=mode, out_dtype=odt)
        assert y.dtype == odt and y.shape == x.shape
        held(kind, where, y, ref, mag, odt)
        if kind != "generic":
            with rcx_env(RCX_FORCE_GENERIC="1"):
                yg = ops.upadd_dwconv(x, cs, wk, bk if bias else None, k=k, mode=mode, out_dtype=odt)
                torch.cuda.synchronize()
            held(f"{kind}/forced-generic", where, yg, ref, mag, odt)


# one test an extent of UP_EXTENTS: its type triples and resize modes, with and without bias
@pytest.mark.parametrize("group", gathered(UP_CASES, lambda case: up_id(case).split("-nearest-")[0].split("-bilinear-")[0]), ids=group_id)
def test_upadd_dwconv_matches_float64(group, held):
    assert len(group[1]) == (len(UP_TRIPLES) * len(MODES) if group[1][0][0][2] is not None else len(UP_PAIRS))
    for case in group[1]:
        up_case(case, held)
    held.finish()


# ---- the grouped Downsample conv of RecNeXt-T / S / B --------------------------------------------------------------------------------------------------------------

GROUPED_CASES = list(itertools.product(GROUPED_SHAPES, DT))


def grouped_id(case):
    shape, dts = case
    return f"{'x'.join(map(str, shape))}-{dts}"


def grouped_inputs(case):
    (n, h, w, cin, cout, g_), dts = case
    g = gen("grouped", grouped_id(case))
    ci = cin // g_
    return rnd(g, (n, cin, h, w), DT[dts]), rnd(g, (cout, ci, 5, 5), F32, (25 * ci) ** -0.5), rnd(g, (cout,), F32, 0.5)


def grouped_case(case, held):
    (n, h, w, cin, cout, groups), dts = case
    dt = DT[dts]
    x32, wt, b = grouped_inputs(case)
    assert ops.grouped_conv2d_supported(n, h, w, cin, cout, groups, 5, 2, dt)
    x, wp, bg = dev(x32, dt), ops.pack_grouped_weight(wt.to("cuda:0")), b.to("cuda:0")
    for bias in (True, False):
        ref, mag = fwd64.grouped_conv2d_fwd64(x32, wt, b if bias else None, groups)
        y = ops.grouped_conv2d(x, wp, bg if bias else None, groups)
        assert y.dtype == dt and tuple(y.shape) == tuple(ref.shape)
        held("as dispatched", f"{grouped_id(case)}-{'bias' if bias else 'nobias'}", y, ref, mag, dt)


# one test a shape: the three I/O types, with and without bias
@pytest.mark.parametrize("group", gathered(GROUPED_CASES, lambda case: "x".join(map(str, case[0]))), ids=group_id)
def test_grouped_conv2d_matches_float64(group, held):
    assert len(group[1]) == len(DT)
    for case in group[1]:
        grouped_case(case, held)
    held.finish()
