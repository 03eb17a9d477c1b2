"""Where the kernels read and write (tests/guard.py), for every launching entry of recnext_amd.ops: one table of cases, five properties each.

  A  nothing outside an allocation is written     B  every output element is written, no unwritten scratch feeds it
  C  nothing outside an input is read             D  inputs are not modified            E  the promised workspace is enough

Every case is (entry, id, build() -> the call's arguments on the GPU, invoke(*arguments) -> tensors); "a+b" names a case that calls two entries in turn.  guard.run_properties first repeats the plain call
and asserts equal bits (every entry here is documented deterministic; the table has no entry held to a looser bar), then runs it with the library's
allocations poisoned and guarded (A, B, and E for every internally allocated workspace: under the proxy each has exactly the size its *_bytes query
returned) and with every tensor argument in a guarded arena of its own, guards 0x00 and 0xFF (C, D).  Raw byte buffers (the saved pyramid of the
training forward) are passed on to the backward, not compared themselves.
"""
import collections
import re
import zlib

import pytest
import torch

from tests import guard

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT_ID = {F32: "f32", BF16: "bf16", F16: "f16"}

Case = collections.namedtuple("Case", "entry id build invoke same")        # same: None = equal bits, else the entry's own parity bar (none needs one)
CASES = []
# entries of the table that are not functions of recnext_amd.ops: one forward + backward through the modules (the autograd Functions' own allocations)
MODULE_ENTRIES = ("module:RecConv2d", "module:RecConv2d-frozen", "module:RecAttn2d", "module:ls_token_half")


def case(entry, cid, build, invoke, same=None):
    CASES.append(Case(entry, f"{entry}-{cid}", build, invoke, same))


def ops():
    from recnext_amd import ops as o
    return o


def gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(tuple(str(k) for k in key)).encode()))


def rnd(g, shape, dtype=F32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def xid(*v):
    return "x".join(str(i) for i in v)


# ---- RecConv2d: forward, training forward + backward, input-only backward ---------------------------------------------------------------------------------

# (N, C, H, W, level, k): the issue's candidates, then the extents that reach the schedules those do not (asked of the plan functions)
RECCONV = [(2, 40, 7, 7, 1, 5), (1, 100, 7, 7, 1, 5), (3, 24, 14, 14, 2, 5), (5, 8, 14, 14, 2, 5), (2, 16, 16, 16, 1, 5), (1, 8, 64, 64, 3, 5),
           (1, 48, 56, 56, 4, 5), (1, 96, 28, 28, 3, 5), (2, 16, 25, 13, 2, 5), (1, 16, 100, 168, 3, 5), (2, 6, 9, 11, 1, 7), (1, 3, 5, 3, 0, 5),
           (1, 16, 128, 128, 4, 5), (1, 16, 112, 112, 5, 5), (8, 16, 14, 14, 2, 5), (2, 8, 32, 32, 2, 5), (1, 24, 28, 28, 3, 5), (2, 16, 14, 14, 1, 5), (1, 128, 28, 28, 3, 5),
           (2, 8, 9, 11, 1, 7), (1, 12, 10, 6, 2, 3)]            # k = 7 and k = 3 at C % 4 == 0: the backwards at the wider and the narrower halo
MODES = ("bilinear", "nearest")

FWD_FAMILIES = {"lanes7", "lanes16", "split", "nested", "plane", "generic", "cpt56", "cpt28", "cpt64", "cpl14", "cpl7"}
BWD_FAMILIES = {"steps", "one-cpl7", "one-cpl14", "tiled+one", "steps+one", "split"}        # "generic" needs RCX_FORCE_GENERIC: not a schedule of valid extents alone
BWD_INPUT_FAMILIES = BWD_FAMILIES - {"split"}                                              # the input-only backward runs one wave per plane, never split


def plan_family(plan):
    """The family of a forward plan string (rcx_recconv2d_fwd_plan); ValueError for one this table does not know."""
    head = plan.split("(")[0]
    if head in ("split", "nested", "plane", "generic"):
        return head
    if head == "lanes":
        w0 = int(re.search(r"<(\d+),", plan).group(1))                  # the kernel's first template argument: the plane width
        for base, fam in ((7, "lanes7"), (16, "lanes16")):
            if w0 % base == 0 and (w0 // base) & (w0 // base - 1) == 0:
                return fam
    if head == "cpt":
        if "ts=16" in plan:
            return "cpt64"
        tile = re.search(r"k_recconv_cpt<(\d+),", plan)
        if tile and tile.group(1) in ("4", "2"):
            return {"4": "cpt56", "2": "cpt28"}[tile.group(1)]
    if head == "cpl":
        return "cpl14" if "cpl14" in plan else "cpl7"
    raise ValueError(f"unknown forward plan {plan!r}: name its family here and give it a guarded case")


def bwd_plan_families(plan):
    if plan == "steps":
        return {"steps"}
    m = re.fullmatch(r"(one|tiled\(levels=\d+\)\+one|steps\+one)\(k_recconv_(?:bwd|adj)_(cpl7|cpl14)(,split)?\)", plan)
    if not m:
        raise ValueError(f"unknown backward plan {plan!r}: name its family here and give it a guarded case")
    kind = {"one": f"one-{m.group(2)}", "steps+one": "steps+one"}.get(m.group(1), "tiled+one")
    return {kind} | ({"split"} if m.group(3) else set())


def recconv_variants():
    """(extent, dtype, mode, bias) of the table: every extent in all three types, mode and bias alternating so that each appears with each type."""
    out = []
    for i, ext in enumerate(RECCONV):
        for j, dt in enumerate((F32, BF16, F16)):
            out.append((ext, dt, MODES[(i + j) % 2], bool((i + j // 2) % 2)))
    return out


def plan_families_hit():
    o = ops()
    fwd, bwd, inp = set(), set(), set()
    for (n, c, h, w, level, k), dt, mode, _ in recconv_variants():
        fwd.add(plan_family(o.recconv2d_plan(n, c, h, w, level, k, mode, dt)))
        if c % 4 == 0:
            bwd |= bwd_plan_families(o.recconv2d_bwd_plan(n, c, h, w, level, k, dt))
            inp |= bwd_plan_families(o.recconv2d_bwd_input_plan(n, c, h, w, level, k, dt))
    return fwd, bwd, inp


def _recconv_args(ext, dt, bias, what):
    n, c, h, w, level, k = ext
    g = gen("recconv", ext, dt, what)
    x = cl(rnd(g, (n, c, h, w), dt))
    wd = rnd(g, (c, 1, k, k), F32, 0.2)
    wc = [rnd(g, (c, 1, k, k), F32, 0.2) for _ in range(level + 1)]
    bd = rnd(g, (c,), F32, 0.1) if bias else None
    bc = [rnd(g, (c,), F32, 0.1) for _ in range(level + 1)] if bias else None
    wpack, bpack, wflip = ops().pack_recconv_params(wd, wc, bd, bc, with_flipped=True)
    gy = cl(rnd(g, (n, c, h, w), dt))
    return x, gy, wpack, bpack, wflip


for _ext, _dt, _mode, _bias in recconv_variants():
    _n, _c, _h, _w, _level, _k = _ext
    _id = f"{xid(*_ext)}-{DT_ID[_dt]}-{_mode}-{'bias' if _bias else 'nobias'}"

    def _b_fwd(ext=_ext, dt=_dt, bias=_bias):
        x, _, wpack, bpack, _ = _recconv_args(ext, dt, bias, "fwd")
        return x, wpack, bpack

    case("recconv2d_forward", _id, _b_fwd, lambda x, wp, bp, level=_level, k=_k, mode=_mode: ops().recconv2d_forward(x, wp, bp, level, k, mode))
    if _c % 4:
        continue                                         # the backward kernels take channel counts that are multiples of 4

    def _b_train(ext=_ext, dt=_dt, bias=_bias):
        x, gy, wpack, bpack, wflip = _recconv_args(ext, dt, bias, "train")
        return x, gy, wpack, bpack, wflip

    def _i_train(x, gy, wpack, bpack, wflip, level=_level, k=_k, mode=_mode, bias=_bias):
        y, saved = ops().recconv2d_forward_train(x, wpack, bpack, level, k, mode)
        gx, gw, gb = ops().recconv2d_backward(x, gy, wpack, saved, level, k, mode, need_bias=bias, wflip=wflip)
        return y, gx, gw, gb

    case("recconv2d_forward_train+recconv2d_backward", _id, _b_train, _i_train)

    def _b_inp(ext=_ext, dt=_dt, bias=_bias):
        _, gy, wpack, _, wflip = _recconv_args(ext, dt, bias, "input")
        return gy, wpack, wflip

    case("recconv2d_input_backward", _id, _b_inp, lambda gy, wp, wf, level=_level, k=_k, mode=_mode: ops().recconv2d_input_backward(gy, wp, wf, level, k, mode))


def _b_param_grads(dt):
    def build():
        ext = (3, 24, 14, 14, 2, 5)
        x, gy, wpack, bpack, wflip = _recconv_args(ext, dt, True, "param_grads")
        return x, gy, wpack, bpack, wflip
    return build


def _i_param_grads(x, gy, wpack, bpack, wflip):
    """The module's form of the backward: the final reduction writes the parameters' gradients in their own layout and type."""
    o = ops()
    y, saved = o.recconv2d_forward_train(x, wpack, bpack, 2, 5, "bilinear")
    gws = o.torch.empty((4, 24, 1, 5, 5), dtype=x.dtype, device=x.device)
    gbs = o.torch.empty((4, 24), dtype=x.dtype, device=x.device)
    gx, _, _ = o.recconv2d_backward(x, gy, wpack, saved, 2, 5, "bilinear", wflip=wflip, param_grads=([gws[i] for i in range(4)], [gbs[i] for i in range(4)]))
    return y, gx, gws, gbs


for _dt in (F32, BF16):
    case("recconv2d_forward_train+recconv2d_backward", f"param_grads-{DT_ID[_dt]}", _b_param_grads(_dt), _i_param_grads)


# ---- single steps and their backwards ------------------------------------------------------------------------------------------------------------------------

STEP_PLANES = [(9, 11), (7, 7), (14, 14), (5, 3), (30, 44)]


def _step_args(c, h, w, k, xdt, what, mult=1, coarse=None, cdt=F32, stride=1, n=2):
    g = gen("step", c, h, w, k, xdt, what, mult, coarse, cdt, stride)
    x = cl(rnd(g, (n, c, h, w), xdt))
    wk = ops().pack_dw_weight(rnd(g, (mult * c, 1, k, k), F32, 0.2))
    b = ops().pack_bias(rnd(g, (mult * c,), F32, 0.1))
    p = k // 2
    ho, wo = (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1
    gy = cl(rnd(g, (n, mult * c, ho, wo), F32))
    cs = cl(rnd(g, (n, c) + tuple(coarse), cdt)) if coarse is not None else None
    return x, cs, gy, wk, b


for _i, (_h, _w) in enumerate(STEP_PLANES):
    for _k in (3, 5, 7):
        for _stride in (1, 2):
            for _j, (_din, _dout) in enumerate([(F32, F32), (BF16, F32), (BF16, BF16), (F32, BF16), (F16, F16)]):
                if (_i + _k // 2 + _stride + _j) % 2:           # half of the cross product: every plane, k, stride and type pair appears several times
                    continue
                _c = 24 if _j % 2 == 0 else 40

                def _b(c=_c, h=_h, w=_w, k=_k, din=_din, stride=_stride):
                    x, _, _, wk, b = _step_args(c, h, w, k, din, "dwconv", stride=stride)
                    return x, wk, b

                case("dwconv2d", f"{xid(_c, _h, _w)}-k{_k}s{_stride}-{DT_ID[_din]}-{DT_ID[_dout]}", _b,
                     lambda x, wk, b, k=_k, stride=_stride, dout=_dout: ops().dwconv2d(x, wk, b, k=k, stride=stride, out_dtype=dout))
            for _xdt in (F32, BF16, F16):
                if (_i + _k + _stride) % 3 != (0 if _xdt == F32 else 1 if _xdt == BF16 else 2) and (_h, _w) != (30, 44):
                    continue

                def _b(h=_h, w=_w, k=_k, xdt=_xdt, stride=_stride):
                    x, _, gy, wk, _ = _step_args(24, h, w, k, xdt, "dwconv_bwd", stride=stride)
                    return x, gy, wk

                case("dwconv2d_backward", f"{xid(24, _h, _w)}-k{_k}s{_stride}-{DT_ID[_xdt]}", _b,
                     lambda x, gy, wk, k=_k, stride=_stride: ops().dwconv2d_backward(x, gy, wk, k, stride, need_bias=True))
                if _xdt != F32 and _k == 5:                      # gy in x's own 16-bit type, as autograd hands it over (the entry widens it before the launch)
                    case("dwconv2d_backward", f"{xid(24, _h, _w)}-k{_k}s{_stride}-{DT_ID[_xdt]}-gy16", _b,
                         lambda x, gy, wk, k=_k, stride=_stride: ops().dwconv2d_backward(x, gy.to(x.dtype), wk, k, stride))

                def _b(h=_h, w=_w, k=_k, xdt=_xdt, stride=_stride):
                    x, _, gy, wk, b = _step_args(6 if h < 10 else 24, h, w, k, xdt, "mult2", mult=2, stride=stride)
                    return x, gy, wk, b

                case("dwconv2d_mult2", f"{xid(_h, _w)}-k{_k}s{_stride}-{DT_ID[_xdt]}", _b,
                     lambda x, gy, wk, b, k=_k, stride=_stride: ops().dwconv2d_mult2(x, wk, b, k=k, stride=stride))
                if _stride == 2:
                    case("dwconv2d_mult2_backward", f"{xid(_h, _w)}-k{_k}-{DT_ID[_xdt]}", _b,
                         lambda x, gy, wk, b, k=_k: ops().dwconv2d_mult2_backward(x, gy, wk, k, need_bias=True))
                    if _xdt != F32 and _k == 5:
                        case("dwconv2d_mult2_backward", f"{xid(_h, _w)}-k{_k}-{DT_ID[_xdt]}-gy16", _b,
                             lambda x, gy, wk, b, k=_k: ops().dwconv2d_mult2_backward(x, gy.to(x.dtype), wk, k))

# conv_k(x + resize(coarse)): the coarse planes of test_upadd_dwconv_piece, the 30 x 44 plane on the tiled kernel, k = 3 / 7 on the generic one
UPADD = [((7, 7), (4, 4)), ((14, 14), (7, 7)), ((9, 11), (5, 6)), ((16, 16), (8, 8)), ((5, 3), (1, 1)), ((30, 44), (15, 22))]
for _i, ((_h, _w), _coarse) in enumerate(UPADD):
    for _j, (_xdt, _cdt, _odt) in enumerate([(F32, F32, F32), (BF16, F32, F32), (BF16, BF16, BF16), (F32, BF16, F32), (F16, F32, F16), (F16, F16, F16)]):
        _k = 5 if (_i + _j) % 3 else (3, 7)[(_i + _j) // 3 % 2]
        _mode = MODES[(_i + _j) % 2]
        _c = (16, 40, 64)[(_i + _j) % 3]

        def _b(c=_c, h=_h, w=_w, k=_k, xdt=_xdt, cdt=_cdt, coarse=_coarse):
            x, cs, _, wk, b = _step_args(c, h, w, k, xdt, "upadd", coarse=coarse, cdt=cdt)
            return x, cs, wk, b

        case("upadd_dwconv", f"{xid(_c, _h, _w)}-k{_k}-{_mode}-{DT_ID[_xdt]}-{DT_ID[_cdt]}-{DT_ID[_odt]}", _b,
             lambda x, cs, wk, b, k=_k, mode=_mode, odt=_odt: ops().upadd_dwconv(x, cs, wk, b, k=k, mode=mode, out_dtype=odt))
        if _cdt != F32:
            continue                                     # the backward takes the coarse plane in float32

        def _b(c=_c, h=_h, w=_w, k=_k, xdt=_xdt, coarse=_coarse):
            x, cs, gy, wk, _ = _step_args(c, h, w, k, xdt, "upadd_bwd", coarse=coarse)
            return x, cs, gy, wk

        case("upadd_dwconv_backward", f"{xid(_c, _h, _w)}-k{_k}-{_mode}-{DT_ID[_xdt]}", _b,
             lambda x, cs, gy, wk, k=_k, mode=_mode: ops().upadd_dwconv_backward(x, cs, gy, wk, k=k, mode=mode, need_bias=True))
        if _xdt != F32:
            case("upadd_dwconv_backward", f"{xid(_c, _h, _w)}-k{_k}-{_mode}-{DT_ID[_xdt]}-gy16", _b,
                 lambda x, cs, gy, wk, k=_k, mode=_mode: ops().upadd_dwconv_backward(x, cs, gy.to(x.dtype), wk, k=k, mode=mode))


def _b_upadd_no_coarse():
    x, _, _, wk, b = _step_args(16, 9, 11, 5, F32, "upadd0")
    return x, wk, b


case("upadd_dwconv", "no-coarse-16x9x11", _b_upadd_no_coarse, lambda x, wk, b: ops().upadd_dwconv(x, None, wk, b, k=5))


# ---- attention cores ---------------------------------------------------------------------------------------------------------------------------------------

def _core_args(b, cqk, cv, h, w, dt, what):
    g = gen("core", b, cqk, cv, h, w, dt, what)
    return rnd(g, (b, h * w, cqk), dt), rnd(g, (b, h * w, cqk), dt), cl(rnd(g, (b, cv, h, w), dt)), cl(rnd(g, (b, cv, h, w), dt))


for (_b_, _c, _heads, _h, _w) in [(2, 16, 4, 4, 4), (2, 224, 8, 7, 7), (9, 32, 1, 3, 3)]:
    for _dt in (F32, BF16, F16):
        _id = f"{xid(_b_, _c, _heads, _h, _w)}-{DT_ID[_dt]}"
        _bld = lambda b=_b_, c=_c, h=_h, w=_w, dt=_dt: _core_args(b, c, c, h, w, dt, "narrow")
        case("linear_attention_core", _id, _bld, lambda q, k, v, pe, heads=_heads: ops().linear_attention_core(q, k, v, pe, heads))
        case("linear_attention_core_backward", _id, _bld, lambda q, k, v, go, heads=_heads: ops().linear_attention_core_backward(q, k, v, go, heads))
        for _bias in (True, False):

            def _b(b=_b_, c=_c, h=_h, w=_w, dt=_dt, bias=_bias):
                q, k, v, _ = _core_args(b, c, c, h, w, dt, "pe")
                g = gen("pe", c)
                return q, k, v, ops().pack_dw_weight(rnd(g, (c, 1, 3, 3), F32, 0.2)), (ops().pack_bias(rnd(g, (c,), F32, 0.1)) if bias else None)

            def _i(q, k, v, wpe, bpe, heads=_heads):
                out = ops().linear_attention_core_pe(q, k, v, wpe, bpe, heads)
                assert out is not None, "linear_attention_core_pe has a kernel for every head size of this table"
                return out

            case("linear_attention_core_pe", f"{_id}-{'bias' if _bias else 'nobias'}", _b, _i)

for _n in (16, 45, 49):
    for _heads in (1, 2):
        for _dk, _dv in [(4, 8), (96, 96), (64, 128), (128, 64)]:
            for _dt in (F32, BF16, F16):
                _h, _w = {16: (4, 4), 45: (5, 9), 49: (7, 7)}[_n]
                _id = f"n{_n}-h{_heads}-{_dk}x{_dv}-{DT_ID[_dt]}"
                _bld = lambda heads=_heads, dk=_dk, dv=_dv, h=_h, w=_w, dt=_dt: _core_args(2, heads * dk, heads * dv, h, w, dt, "wide")
                case("linear_attention_wide", _id, _bld, lambda q, k, v, pe, heads=_heads: ops().linear_attention_wide(q, k, v, pe, heads))
                case("linear_attention_wide_backward", _id, _bld, lambda q, k, v, go, heads=_heads: ops().linear_attention_wide_backward(q, k, v, go, heads))


# ---- matrix-core attention units ---------------------------------------------------------------------------------------------------------------------------

def _attn_packs(g, c, bias, convs=0):
    o = ops()
    out = []
    for _ in range(convs):
        out += [o.pack_dw_weight(rnd(g, (c, 1, 5, 5), F32, 0.2)), o.pack_bias(rnd(g, (c,), F32, 0.1)) if bias else None]
    wqk = rnd(g, (2 * c, c // 2), F32, (2.0 / c) ** 0.5).to(BF16).contiguous()
    return out, [wqk, rnd(g, (2 * c,), F32, 0.1), o.pack_dw_weight(rnd(g, (c, 1, 3, 3), F32, 0.2)), o.pack_bias(rnd(g, (c,), F32, 0.1)) if bias else None]


# (B, C, heads, h, w): one launch up to 64 tokens, two above (A5's 40-wide heads at 14 x 14: 196 tokens; 2 x 64 x 9 x 11: 99)
QKCORE = [(9, 32, 1, 3, 3), (2, 256, 8, 5, 9), (3, 320, 8, 7, 7), (2, 160, 4, 14, 14), (2, 512, 16, 4, 4), (2, 64, 2, 9, 11)]
for _cs in QKCORE:
    for _bias in (True, False):
        def _b(cs=_cs, bias=_bias):
            b, c, heads, h, w = cs
            g = gen("qkcore", cs, bias)
            assert ops().recattn_qkcore_supported(c, heads, h, w)
            return (cl(rnd(g, (b, c, h, w), F32)), *_attn_packs(g, c, bias)[1])

        case("recattn_qkcore", f"{xid(*_cs)}-{'bias' if _bias else 'nobias'}", _b, lambda d, wqk, bqk, wpe, bpe, heads=_cs[2]: ops().recattn_qkcore(d, wqk, bqk, wpe, bpe, heads))

for _cs in [(5, 32, 1, 7), (3, 320, 8, 14), (2, 320, 8, 7), (2, 512, 16, 7), (2, 64, 2, 14)]:
    for _xdt in (BF16, F16):
        for _bias in (True, False):
            def _b(cs=_cs, xdt=_xdt, bias=_bias):
                b, c, heads, hw = cs
                g = gen("down_qkcore", cs, xdt, bias)
                assert ops().recattn_down_qkcore_supported(c, heads, hw, hw, xdt)
                conv, rest = _attn_packs(g, c, bias, convs=1)
                return (cl(rnd(g, (b, c, hw, hw), xdt)), *conv, *rest)

            case("recattn_down_qkcore", f"{xid(*_cs)}-{DT_ID[_xdt]}-{'bias' if _bias else 'nobias'}", _b,
                 lambda x, wd, bd, wqk, bqk, wpe, bpe, heads=_cs[2]: ops().recattn_down_qkcore(x, wd, bd, wqk, bqk, wpe, bpe, heads))

for _cs in [(5, 32, 1, 7), (3, 256, 8, 14), (2, 40, 2, 14), (3, 512, 16, 7), (2, 96, 4, 7)]:
    for _xdt in (BF16, F16):
        for _bias in (True, False):
            def _b(cs=_cs, xdt=_xdt, bias=_bias):
                b, c, heads, hw = cs
                g = gen("recattn2d", cs, xdt, bias)
                assert ops().recattn2d_supported(c, heads, hw, hw, "nearest", xdt)
                conv, rest = _attn_packs(g, c, bias, convs=2)
                return (cl(rnd(g, (b, c, hw, hw), xdt)), *conv[:2], *rest, *conv[2:])

            case("recattn2d", f"{xid(*_cs)}-{DT_ID[_xdt]}-{'bias' if _bias else 'nobias'}", _b,
                 lambda x, wd, bd, wqk, bqk, wpe, bpe, wc, bc, heads=_cs[2]: ops().recattn2d(x, wd, bd, wqk, bqk, wpe, bpe, wc, bc, heads))


# ---- channel MLP, all three kernel forms, and the aliased call z is x ----------------------------------------------------------------------------------------

def _mlp_shapes():
    from tests.test_mlp512_gpu import _cases
    wide = _cases()
    return [(1, 64, 128, 1, 1), (2, 40, 80, 13, 7), (1, 80, 150, 5, 5), (1, 256, 512, 3, 5), (7, 256, 512, 13, 11), (2, 256, 480, 14, 14), (1, 320, 600, 5, 3),
            wide["ragged"], wide["hidden960"]]


MLP_IDS = ["1x64x128x1x1", "2x40x80x13x7", "1x80x150x5x5", "1x256x512x3x5", "7x256x512x13x11", "2x256x480x14x14", "1x320x600x5x3", "wide-ragged", "wide-hidden960"]


def _b_mlp(index, alias):
    def build():
        n, c, hid, h, w = _mlp_shapes()[index]
        o = ops()
        g = gen("mlp", index)
        hp = o.channel_mlp_hidden(n * h * w, c, hid, BF16)
        assert hp > 0, (n, c, hid, h, w)
        wfrag, bias, hp = o.pack_channel_mlp(rnd(g, (hid, c), BF16, (2.0 / c) ** 0.5), rnd(g, (hid,), BF16, 0.3), rnd(g, (c, hid), BF16, (1.0 / hid) ** 0.5),
                                             rnd(g, (c,), BF16, 0.3), hidden_to=hp)
        z = cl(rnd(g, (n, c, h, w), BF16))
        x = z if alias else cl(rnd(g, (n, c, h, w), BF16))
        return z, x, wfrag, bias, hp
    return build


for _i, _id in enumerate(MLP_IDS):
    for _alias in (False, True):
        case("channel_mlp", _id + ("-aliased" if _alias else ""), _b_mlp(_i, _alias), lambda z, x, wfrag, bias, hp: ops().channel_mlp(z, x, wfrag, bias, hp))


# ---- stem: the ragged tiles of tests/test_stem_tiles_gpu.py, the smallest input and a non-square one ---------------------------------------------------------

def _stem_cases():
    from tests.test_stem_tiles_gpu import CASES as TILES
    return list(TILES) + [(1, 24, 48, 1, 1), (2, 32, 64, 7, 30)]


for _cs in _stem_cases():
    def _b(cs=_cs):
        n, cm, co, h, w = cs
        o = ops()
        g = gen("stem", cs)
        assert o.stem_supported(n, h, w, cm, co, BF16), cs
        packs = o.pack_stem(rnd(g, (cm, 3, 3, 3), BF16, (2.0 / 27) ** 0.5), rnd(g, (cm,), BF16, 0.3), rnd(g, (co, cm, 3, 3), BF16, (2.0 / (9 * cm)) ** 0.5), rnd(g, (co,), BF16, 0.3))
        return (cl(rnd(g, (n, 3, h, w), BF16)), *packs, cm, co)

    case("stem", xid(*_cs), _b, lambda x, w1p, b1p, w2f, b2p, cm, co: ops().stem(x, w1p, b1p, w2f, b2p, cm, co))


# ---- the LS token half: the fixtures' parameters, one-workgroup and tiled entries, the caller's exact-size workspace (E) ---------------------------------------

LS_PLANES = [(1, 1), (3, 5), (2, 65), (9, 13), (25, 19)]
# (entry, fixture loader, fixture): each runs on the fixture's own square plane and on every plane of LS_PLANES its support query accepts
LS = [("ls_recattn", "block", "7x7_c256"), ("ls_recattn", "block", "14x14_c128"), ("ls_la3", "block", "4x4_c512"),
      ("ls_recattn_tiled", "tiled", "36x36_c128"), ("ls_recattn_tiled", "tiled", "16x16_c384"), ("ls_la3_tiled", "tiled", "12x12_c512")]
_LS_MODULES, _LS_BLOCKS = {}, {}


def _ls_module(kind, name):
    """(block on the CPU, fixture's plane, C, split, heads as the entries take them, is it LinearAttention3): no GPU needed, the table is built from it."""
    from tests.test_ls_tiled_cpu import load_tiled_block
    from tests.test_lsnet_cpu import build_block, load_block
    if (kind, name) not in _LS_MODULES:
        _, _, _, sd, meta = (load_block if kind == "block" else load_tiled_block)(name)
        blk = build_block(meta, sd)
        attn = blk.token_mixer.attn
        la3 = type(attn).__name__ == "LinearAttention3"
        _LS_MODULES[(kind, name)] = (blk, (meta["H"], meta["W"]), meta["C"], blk.token_mixer.split_idx, attn.num_heads if la3 else attn.down[1].num_heads, la3)
    return _LS_MODULES[(kind, name)]


def _ls_block(kind, name):
    if (kind, name) not in _LS_BLOCKS:
        blk, _, c, s, heads, la3 = _ls_module(kind, name)
        blk = blk.to(DEV)
        with torch.no_grad():
            packs = blk.packed_params()
        _LS_BLOCKS[(kind, name)] = (packs, c, s, heads, la3)
    return _LS_BLOCKS[(kind, name)]


def _ls_case(entry, kind, name, plane, batch, dt, own_ws):
    def build():
        packs, c, s, heads, la3 = _ls_block(kind, name)
        assert la3 == ("la3" in entry)
        h, w = plane
        o = ops()
        assert getattr(o, entry + "_supported")(batch, h, w, c, s, heads, dt), (entry, plane)
        x = cl(rnd(gen("ls", entry, name, plane, batch, dt), (batch, c, h, w), dt))
        return (x, *packs, s, heads)

    def invoke(x, *rest):
        o = ops()
        fn = getattr(o, entry)
        if not own_ws:
            return fn(x, *rest)
        # E: the caller's workspace, exactly as large as the query promises, poisoned and guarded (under guarded_library: o.torch is the proxy)
        b, c, h, w = x.shape
        nbytes = getattr(o._lib.load(), f"rcx_{entry}_workspace_bytes")(b, h, w, c, rest[-2], rest[-1], o._DT[x.dtype])
        assert nbytes % 4 == 0
        return fn(x, *rest, workspace=o.torch.empty(nbytes // 4, dtype=F32, device=x.device))

    case(entry, f"{name}-{xid(*plane)}-b{batch}-{DT_ID[dt]}" + ("-own-workspace" if own_ws else ""), build, invoke)


LS_VARIANTS = ((1, F32), (3, BF16), (3, F32), (1, BF16))


def _ls_supported_planes(entry, kind, name):
    """The fixture's own plane, then the planes of LS_PLANES the entry's own support query accepts (asked of the library, for every batch and type of
    the table): the one-workgroup kernels are bounded by 64 tokens (la3) and by the LDS image of one plane (recattn), the tiled ones take them all."""
    _, square, c, s, heads, _ = _ls_module(kind, name)
    query = getattr(ops(), entry + "_supported")
    return [p for p in [square] + LS_PLANES if all(query(b, p[0], p[1], c, s, heads, dt) for b, dt in LS_VARIANTS)]


for _entry, _kind, _name in LS:
    for _pi, _plane in enumerate(_ls_supported_planes(_entry, _kind, _name)):
        for _batch, _dt in LS_VARIANTS[:2] if _pi % 2 == 0 else LS_VARIANTS[2:]:
            _ls_case(_entry, _kind, _name, _plane, _batch, _dt, False)
            if _entry.endswith("_tiled"):
                _ls_case(_entry, _kind, _name, _plane, _batch, _dt, True)


# ---- packing launches ------------------------------------------------------------------------------------------------------------------------------------------

for _c in (6, 100):
    for _k in (3, 7):
        for _dt in (BF16, F32):
            _id = f"c{_c}-k{_k}-{DT_ID[_dt]}"
            case("pack_dw_weight", _id, lambda c=_c, k=_k, dt=_dt: (rnd(gen("pw", c, k), (c, 1, k, k), dt),), lambda w: ops().pack_dw_weight(w))
            case("pack_bias", _id, lambda c=_c, k=_k, dt=_dt: (rnd(gen("pb", c, k), (c,), dt),), lambda b: ops().pack_bias(b))
            # out=: the caller's destination, exactly k k C / C floats (under guarded_library ops().torch is the proxy: poisoned and guarded)
            case("pack_dw_weight", _id + "-out", lambda c=_c, k=_k, dt=_dt: (rnd(gen("pw", c, k), (c, 1, k, k), dt),),
                 lambda w: ops().pack_dw_weight(w, out=ops().torch.empty(w.numel(), dtype=F32, device=w.device)))
            case("pack_bias", _id + "-out", lambda c=_c, k=_k, dt=_dt: (rnd(gen("pb", c, k), (c,), dt),),
                 lambda b: ops().pack_bias(b, out=ops().torch.empty(b.numel(), dtype=F32, device=b.device)))
            for _flip in (False, True):
                for _bias in (False, True):
                    def _b(c=_c, k=_k, dt=_dt, bias=_bias):
                        g = gen("prp", c, k, dt)
                        return (rnd(g, (c, 1, k, k), dt), [rnd(g, (c, 1, k, k), dt) for _ in range(3)], rnd(g, (c,), dt) if bias else None,
                                [rnd(g, (c,), dt) for _ in range(3)] if bias else None)

                    case("pack_recconv_params", f"{_id}-{'flipped' if _flip else 'plain'}-{'bias' if _bias else 'nobias'}", _b,
                         lambda wd, wc, bd, bc, flip=_flip: tuple(t for t in ops().pack_recconv_params(wd, wc, bd, bc, with_flipped=flip) if t is not None))
        case("unpack_recconv_grads", f"c{_c}-k{_k}", lambda c=_c, k=_k: (rnd(gen("ug", c, k), (4, k * k * c), F32),), lambda gw, c=_c, k=_k: ops().unpack_recconv_grads(gw, 4, c, k))


# ---- through the modules: the autograd Functions' own allocations ------------------------------------------------------------------------------------------------

def _module_step(mod, x, gy):
    for m in mod.modules():
        if hasattr(m, "_pack_key"):
            m._pack_key = None                       # pack again: the packs are allocations of this call too
    for p in mod.parameters():
        p.grad = None
    x = x.detach().requires_grad_(True)
    y = mod(x)
    y = y[1] if isinstance(y, tuple) else y
    y.backward(gy)
    torch.cuda.synchronize()
    return (y.detach(), x.grad) + tuple(p.grad for p in mod.parameters() if p.grad is not None)


def _b_recconv_module(dt, frozen):
    def build():
        import recnext_amd
        torch.manual_seed(5)
        mod = recnext_amd.RecConv2d(24, kernel_size=5, level=2, bias=True).to(DEV).to(dt).train()
        if frozen:
            mod.requires_grad_(False)
        g = gen("module", dt)
        return mod, cl(rnd(g, (3, 24, 14, 14), dt)), cl(rnd(g, (3, 24, 14, 14), dt))
    return build


def _b_recattn_module():
    import recnext_amd.recattn
    torch.manual_seed(6)
    mod = recnext_amd.recattn.RecAttn2d(64, num_heads=2, stage=2).to(DEV).train()
    g = gen("recattn module")
    return mod, cl(rnd(g, (2, 64, 14, 14))), cl(rnd(g, (2, 64, 14, 14)))


class _TokenHalf(torch.nn.Module):
    def __init__(self, blk):
        super().__init__()
        self.blk = blk

    def forward(self, x):
        return self.blk.token_half(x)


def _b_ls_module():
    from tests.test_lsnet_cpu import build_block, load_block
    _, _, _, sd, meta = load_block("7x7_c256")
    blk = build_block(meta, sd).to(DEV).train()
    blk.channel_mixer.requires_grad_(False)
    g = gen("ls module")
    return _TokenHalf(blk), cl(rnd(g, (2, meta["C"], 7, 7))), cl(rnd(g, (2, meta["C"], 7, 7)))


case("module:RecConv2d", "f32", _b_recconv_module(F32, False), _module_step)
case("module:RecConv2d", "bf16", _b_recconv_module(BF16, False), _module_step)
case("module:RecConv2d-frozen", "bf16", _b_recconv_module(BF16, True), _module_step)
case("module:RecAttn2d", "f32", _b_recattn_module, _module_step)
case("module:ls_token_half", "f32", _b_ls_module, _module_step)


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_every_plan_family_has_a_guarded_case():
    """The RecConv2d cases reach every schedule family the three plan functions can return for valid extents.  The families are the issue's list, and
    plan_family / bwd_plan_families raise on a plan string they cannot place in it: a schedule with a new head, a lanes kernel on a plane width that
    is neither 7 * 2^k nor 16 * 2^k, or a cpt tile other than the three here fails until it is named and given a case.  A new kernel inside a known
    family (another width of the same lanes form, say) is not told apart: it needs its extent added to RECCONV by hand."""
    fwd, bwd, inp = plan_families_hit()
    assert fwd == FWD_FAMILIES, (sorted(FWD_FAMILIES - fwd), sorted(fwd - FWD_FAMILIES))
    assert bwd == BWD_FAMILIES, (sorted(BWD_FAMILIES - bwd), sorted(bwd - BWD_FAMILIES))
    assert inp == BWD_INPUT_FAMILIES, (sorted(BWD_INPUT_FAMILIES - inp), sorted(inp - BWD_INPUT_FAMILIES))


def test_the_ls_planes_are_the_ones_the_kernels_accept():
    """The tiled entries take every plane of LS_PLANES; the one-workgroup entries take the small ones, and of the ragged odd-width ones whatever
    their support query accepts (no plane is left out by hand)."""
    taken = collections.defaultdict(set)
    for c in CASES:
        for entry, _, name in LS:
            if c.id.startswith(f"{entry}-{name}-"):
                taken[(entry, name)].add(c.id[len(f"{entry}-{name}-"):].split("-")[0])
    for entry, kind, name in LS:
        _, _, ch, s, heads, _ = _ls_module(kind, name)
        want = {xid(*p) for p in LS_PLANES if entry.endswith("_tiled") or all(getattr(ops(), entry + "_supported")(b, p[0], p[1], ch, s, heads, dt) for b, dt in LS_VARIANTS)}
        assert want <= taken[(entry, name)], (entry, name, sorted(want - taken[(entry, name)]))
        assert {"1x1", "3x5"} <= taken[(entry, name)]
        assert entry.endswith("_tiled") or entry == "ls_la3" or {"2x65", "9x13"} <= taken[(entry, name)], (entry, name)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_guard_bands(c):
    with torch.no_grad() if not c.entry.startswith("module:") else torch.enable_grad():
        args = c.build()
        torch.cuda.synchronize()
        guard.run_properties(c.invoke, args, same=c.same)
