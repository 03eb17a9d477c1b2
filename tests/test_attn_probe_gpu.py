"""GPU: every linear-attention kernel against float64, element by element, on inputs in which every token counts (tests/attn_probe.py: the live-key,
unity and two-impulse probes, and dense inputs under the absolute-value form of the bound).  Each test first asserts, through the library's own
queries, that the entry point it names is the one that runs, and records the worst err / bound per output as a test property.

Which kernel an entry point launches (rcx_attn.hip: linattn_core, linattn_core_bwd):
  forward   k_linattn_mfma where D = 32, 16-bit I/O and n >= 512 (there linear_attention_core_pe has no kernel and returns None: the query used
            here), else k_linattn_core4 where D % 4 == 0 (linear_attention_core_fuses_pe), else k_linattn_core;
  backward  k_linattn_bwd_mfma where D = 32 and 16-bit I/O at ANY token count, else k_linattn_bwd.
"""
import zlib

import pytest
import torch

from recnext_amd import _lib, ops
from tests import attn_probe as ap

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DEV = "cuda:0"
LW_TT = ap.kernel_constant("rcx_attnw.hip", "LW_TT")        # tokens per LDS tile, read from the kernels' sources
LA_TT = ap.kernel_constant("rcx_attn.hip", "LA_TT")
LM_NW = ap.kernel_constant("rcx_attn.hip", "LM_NW")         # waves the matrix-core kernels deal the tokens over (steps of 16 and 32 tokens)


def _one_past(tile):
    """A plane of tile + 1 tokens, three rows high where that divides."""
    return (3, (tile + 1) // 3) if (tile + 1) % 3 == 0 else (1, tile + 1)


@pytest.fixture
def ratios(record_property):
    """Every output's worst err / bound as a test property (in the junit report), like tests/test_backward_f64_gpu.py."""
    seen = {}

    def add(name, r):
        seen[name] = max(r, seen.get(name, 0.0))
    yield add
    if seen:
        record_property("worst_ratio", max(seen.values()))
        record_property("ratios", {k: round(v, 3) for k, v in seen.items()})


def _nchw(t, h, w):
    """(B, n, C) token-major -> logical B x C x h x w over the same storage (channels_last)."""
    return t.reshape(t.shape[0], h, w, t.shape[2]).permute(0, 3, 1, 2)


def _tok(y):
    b, c, h, w = y.shape
    return y.permute(0, 2, 3, 1).reshape(b, h * w, c)


def _seed(*xs):
    return zlib.crc32("|".join(map(str, xs)).encode()) % (2 ** 31)


def _fwd_kernel(n, d, dtype):
    if d % 4:
        return "k_linattn_core"
    return "k_linattn_mfma" if d == 32 and dtype != torch.float32 and n >= 512 else "k_linattn_core4"


def _bwd_kernel(d, dtype):
    return "k_linattn_bwd_mfma" if d == 32 and dtype != torch.float32 else "k_linattn_bwd"


def _zero_taps(c):
    return torch.zeros(9 * c, dtype=torch.float32, device=DEV)


def _assert_core_route(kernel, heads, d, h, w, dtype):
    """The library's queries agree with the kernel this case is named after."""
    c = heads * d
    assert ops.linear_attention_core_fuses_pe(c, heads) == (kernel != "k_linattn_core")
    if kernel != "k_linattn_core":
        z = torch.zeros(1, h * w, c, dtype=dtype, device=DEV)
        fused = ops.linear_attention_core_pe(z, z, _nchw(z, h, w), _zero_taps(c), None, heads)
        assert (fused is None) == (kernel == "k_linattn_mfma"), "the case no longer reaches the kernel it is named after"


def _probe(kind, heads, dk, dv, h, w, dtype, every=None, bsz=3):
    n = h * w
    seed = _seed(kind, heads, dk, dv, h, w, dtype)
    if kind == "live":
        return ap.live_key(ap.token_list(n, waves=LM_NW, every=every, seed=seed), n, heads, dk, dv, dtype, DEV, seed, per_head=True)
    if kind == "unity":
        return ap.unity(bsz, n, heads, dk, dv, dtype, DEV, seed)
    return ap.dense(bsz, n, heads, dk, dv, dtype, DEV, seed)


def _check_forward(run, kind, p, heads, dk, kernel, op_dtype, out_dtype, ratios, tag):
    n = p["qpre"].shape[1]
    r = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], heads)
    mag = (r["out"] - p["pe"].double()).abs() if kind != "dense" else (r["M_u"] + r["u"].abs()) / r["w"]
    rel = ap.fwd_rel(kernel, n, dk, op_dtype)
    ratios(tag, ap.assert_within(run(p), r["out"], mag, rel, out_dtype, tag))


# ---- rcx_attn.hip, forward ------------------------------------------------------------------------------------------------------------------

CORE = [(d, h, w, dts, None) for (d, h, w) in [(10, 5, 9), (6, 9, 11)] for dts in ("f32", "bf16")]                                # k_linattn_core, G = 1
CORE += [(d, h, w, dts, None) for (d, h, w) in [(12, 5, 9), (32, 7, 7), (32, 9, 9), (32, 14, 14), (64, 7, 7), (64, 13, 5)]       # k_linattn_core4<32> / <64>
         for dts in ("f32", "bf16", "f16")]
CORE += [(32, h, w, dts, every) for (h, w, every) in [(19, 27, True), (23, 23, True), (28, 28, True), (56, 56, False)]           # k_linattn_mfma
         for dts in ("bf16", "f16")]


@pytest.mark.parametrize("kind", ["live", "unity", "dense"])
@pytest.mark.parametrize("case", CORE, ids=lambda c: f"2x{c[0]}-{c[1]}x{c[2]}-{c[3]}")
def test_linear_attention_core(case, kind, ratios):
    d, h, w, dts, every = case
    dtype, heads, n = DT[dts], 2, h * w
    kernel = _fwd_kernel(n, d, dtype)
    assert kernel == ("k_linattn_core" if d in (10, 6) else "k_linattn_mfma" if every is not None else "k_linattn_core4")
    _assert_core_route(kernel, heads, d, h, w, dtype)
    p = _probe(kind, heads, d, d, h, w, dtype, every=True if every is None else every)
    run = lambda q: _tok(ops.linear_attention_core(q["qpre"], q["kpre"], _nchw(q["v"], h, w), _nchw(q["pe"], h, w), heads))
    _check_forward(run, kind, p, heads, d, kernel, dtype, dtype, ratios, f"{kernel}/{kind}")


def test_an_image_does_not_depend_on_its_batch():
    """The shard property on probe data: image 0 of the live-key batch at 19 x 27 (the matrix-core kernel) alone, bit for bit."""
    h, w, heads, d = 19, 27, 2, 32
    for dtype in (torch.bfloat16, torch.float16):
        p = _probe("live", heads, d, d, h, w, dtype, every=True)
        run = lambda s: ops.linear_attention_core(p["qpre"][s].contiguous(), p["kpre"][s].contiguous(), _nchw(p["v"][s].contiguous(), h, w),
                                                  _nchw(p["pe"][s].contiguous(), h, w), heads)
        whole = run(slice(None))
        for i in (0, 256, 512):
            assert torch.equal(run(slice(i, i + 1))[0], whole[i]), f"image {i} alone differs from image {i} of the batch"


PE_CASES = [(32, 7, 7), (32, 14, 14), (64, 7, 7)]


@pytest.mark.parametrize("kind", ["live", "unity"])
@pytest.mark.parametrize("dts", ["f32", "bf16"])
@pytest.mark.parametrize("case", PE_CASES, ids=lambda c: f"2x{c[0]}-{c[1]}x{c[2]}")
def test_linear_attention_core_pe(case, dts, kind, ratios):
    """pe computed inside the kernel: zero taps and a bias pack (a real pe next to the poison would drown the attention term in the output's
    own rounding; the dense tests cover the conv)."""
    d, h, w = case
    dtype, heads = DT[dts], 2
    assert ops.linear_attention_core_fuses_pe(heads * d, heads)
    p = _probe(kind, heads, d, d, h, w, dtype, every=True)
    bias = ap._away(ap._gen(DEV, d + h), (heads * d,), torch.bfloat16, 0.25).float()
    p["pe"] = bias.expand_as(p["v"]).to(dtype)                                              # bfloat16 values of at most 8 bits: exact in float16 too
    assert torch.equal(p["pe"].float(), bias.expand_as(p["v"]))

    def run(q):
        out = ops.linear_attention_core_pe(q["qpre"], q["kpre"], _nchw(q["v"], h, w), _zero_taps(heads * d), bias, heads)
        assert out is not None, "linear_attention_core_pe has no kernel here"
        return _tok(out)
    _check_forward(run, kind, p, heads, d, "k_linattn_core4", dtype, dtype, ratios, f"k_linattn_core4+pe/{kind}")


# ---- rcx_attnw.hip, forward -----------------------------------------------------------------------------------------------------------------

WIDE_PLANES = [(4, 4), (5, 9), (7, 7), _one_past(LW_TT)]                                    # the last: one token past a token tile


@pytest.mark.parametrize("kind", ["live", "unity", "dense"])
@pytest.mark.parametrize("dts", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("dims", [(4, 8), (32, 64), (64, 128), (128, 64), (96, 96)], ids=lambda d: f"{d[0]}x{d[1]}")
def test_linear_attention_wide(dims, heads, dts, kind, ratios):
    dk, dv = dims
    dtype = DT[dts]
    for h, w in WIDE_PLANES:
        p = _probe(kind, heads, dk, dv, h, w, dtype, every=True)
        assert ops.linear_attention_wide_supported(p["qpre"].shape[0], h * w, heads * dk, heads * dv, heads, dtype)
        run = lambda q: _tok(ops.linear_attention_wide(q["qpre"], q["kpre"], _nchw(q["v"], h, w), _nchw(q["pe"], h, w), heads))
        _check_forward(run, kind, p, heads, dk, "k_linattn_wide_fwd", dtype, dtype, ratios, f"k_linattn_wide_fwd/{kind}/{h}x{w}")


# ---- rcx_qkcore.hip ---------------------------------------------------------------------------------------------------------------------------

def _check_gate(run, p, heads, d, n, ratios, tag):
    r, pe = ap.gate_reference(p, heads)
    mag = (r["out"] - pe).abs()
    rel = ap.fwd_rel("rcx_qkcore", n, d, torch.bfloat16)
    ratios(tag, ap.assert_within(run(p), r["out"], mag, rel, torch.float32, tag))
    return r


QK_CASES = [(d, h, w, True) for d in (20, 24, 28, 32, 36, 40, 48, 60, 64) for (h, w) in [(5, 9), (7, 7), (9, 11)]]
QK_CASES += [(d, 28, 28, False) for d in (20, 24, 28, 32, 36, 40, 48, 60, 64)] + [(40, 19, 27, False), (64, 19, 27, False)]


@pytest.mark.parametrize("kind", ["live", "unity"])
@pytest.mark.parametrize("case", QK_CASES, ids=lambda c: f"2x{c[0]}-{c[1]}x{c[2]}")
def test_recattn_qkcore(case, kind, ratios):
    d, h, w, every = case
    heads, n, c = 2, h * w, 2 * d
    assert ops.recattn_qkcore_supported(c, heads, h, w)
    seed = _seed("qk", kind, d, h, w)
    if kind == "live":
        p = ap.gate_live_key(ap.token_list(n, every=every, seed=seed), n, heads, d, DEV, seed)
    else:
        p = ap.gate_unity(3, n, heads, d, DEV, seed)
    launches = _lib.load().rcx_recattn_qkcore_launches(p["d"].shape[0], h, w, c, heads)
    assert launches == (1 if n <= 64 else 2), f"{launches} launches at {n} tokens"
    run = lambda q: _tok(ops.recattn_qkcore(_nchw(q["d"], h, w), q["wqk"], q["bqk"], _zero_taps(c), q["b_pe"], heads))
    r = _check_gate(run, p, heads, d, n, ratios, f"rcx_qkcore({launches})/{kind}")
    if kind == "live":                                                                      # v = d: the gate channel's own attention term is +1
        gate = r["out"][..., c - 1] - p["b_pe"][c - 1].double()
        assert float((gate - 1).abs().max()) <= 7e-5


@pytest.mark.parametrize("xdts", ["bf16", "f16"])
@pytest.mark.parametrize("heads,d", [(2, 40), (4, 40), (2, 64)])
def test_recattn_down_qkcore(heads, d, xdts, ratios):
    """The live key through the centre-tap down conv: x carries the probe on its even pixels and more poison on the others."""
    xdt, c, hw, hc = DT[xdts], heads * d, 14, 7
    assert ops.recattn_down_qkcore_supported(c, heads, hw, hw, xdt)
    n = hc * hc
    seed = _seed("down", heads, d, xdts)
    p = ap.gate_live_key(list(range(n)), n, heads, d, DEV, seed, dtype=xdt)
    bsz = n
    x = ap._rn(ap._gen(DEV, seed + 1), (bsz, hw, hw, c), xdt, ap.POISON)
    x[:, ::2, ::2] = p["d"].reshape(bsz, hc, hc, c).to(xdt)
    assert torch.equal(x[:, ::2, ::2].float().reshape(bsz, n, c), p["d"])
    wdn = torch.zeros(25, c, dtype=torch.float32, device=DEV)
    wdn[12] = 1.0
    run = lambda q: _tok(ops.recattn_down_qkcore(x.permute(0, 3, 1, 2), wdn.reshape(-1), None, q["wqk"], q["bqk"], _zero_taps(c), q["b_pe"], heads))
    _check_gate(run, p, heads, d, n, ratios, "rcx_down_qkcore/live")


# ---- backward ---------------------------------------------------------------------------------------------------------------------------------

def _check_backward(fn, p, heads, dk, dv, h, w, dtype, kernel, ratios, tag):
    n = h * w
    ref, T = ap.grads64(p["qpre"], p["kpre"], p["v"], p["gout"], heads)
    q, k = p["qpre"].clone().requires_grad_(True), p["kpre"].clone().requires_grad_(True)
    v = _nchw(p["v"], h, w).detach().requires_grad_(True)
    out = fn.apply(q, k, v, _nchw(p["pe"], h, w), heads)
    gq, gk, gv = torch.autograd.grad(out, [q, k, v], _nchw(p["gout"], h, w))
    for name, got in (("gq", gq), ("gk", gk), ("gv", _tok(gv))):
        assert got.dtype == dtype
        rel = ap.bwd_rel(kernel, name, n, dk, dv, dtype)
        ratios(f"{tag}/{name}", ap.assert_within(got, ref[name], T[name], rel, dtype, f"{tag} {name}"))


def _impulses(pairs, heads, dk, dv, h, w, dtype):
    return ap.two_impulses(pairs, h * w, heads, dk, dv, dtype, DEV, _seed("imp", dk, dv, h, w, dtype))


def _dense_bwd(heads, dk, dv, h, w, dtype):
    return ap.dense(3, h * w, heads, dk, dv, dtype, DEV, _seed("dense-bwd", dk, dv, h, w, dtype))


@pytest.mark.parametrize("kind", ["impulses", "dense"])
@pytest.mark.parametrize("dts", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", [(12, 5, 9), (32, 7, 7), (32, 9, 9), (64, 13, 5)], ids=lambda c: f"2x{c[0]}-{c[1]}x{c[2]}")
def test_linear_attention_core_backward(case, dts, kind, ratios):
    """k_linattn_bwd, except that linattn_core_bwd (rcx_attn.hip) sends 32-wide heads in 16 bits to k_linattn_bwd_mfma at ANY token count.  So at
    D = 32 k_linattn_bwd is probed in float32 only (no 16-bit D = 32 call can reach it; D = 12 and 64 probe its 16-bit loads and stores), and the
    bf16 / f16 cases at 7 x 7 and 9 x 9 are the matrix-core kernel's small planes: their impulse pairs come from the edges of ITS 16- and 32-token
    steps (0, 15, 16, 31, 32, 47, 48, ...), squared, not from the vector kernel's 64-token tile."""
    d, h, w = case
    dtype, heads, n = DT[dts], 2, h * w
    kernel = _bwd_kernel(d, dtype)
    _assert_core_route(_fwd_kernel(n, d, dtype), heads, d, h, w, dtype)
    if kind == "impulses":
        edges = ap.step_edges(n) if kernel == "k_linattn_bwd_mfma" else ap.edge5(n, LA_TT)
        p = _impulses(ap.impulse_pairs(n, seed=n, edges=edges), heads, d, d, h, w, dtype)
    else:
        p = _dense_bwd(heads, d, d, h, w, dtype)
    _check_backward(ops.LinearAttentionCoreFn, p, heads, d, d, h, w, dtype, kernel, ratios, f"{kernel}/{kind}")


@pytest.mark.parametrize("kind", ["impulses", "dense"])
@pytest.mark.parametrize("dts", ["bf16", "f16"])
@pytest.mark.parametrize("h,w", [(19, 27), (28, 28)])
def test_linear_attention_core_backward_mfma(h, w, dts, kind, ratios):
    dtype, heads, d, n = DT[dts], 2, 32, h * w
    assert _bwd_kernel(d, dtype) == "k_linattn_bwd_mfma"
    _assert_core_route("k_linattn_mfma", heads, d, h, w, dtype)
    p = _impulses(ap.impulse_pairs(n, seed=n, every=True), heads, d, d, h, w, dtype) if kind == "impulses" else _dense_bwd(heads, d, d, h, w, dtype)
    _check_backward(ops.LinearAttentionCoreFn, p, heads, d, d, h, w, dtype, "k_linattn_bwd_mfma", ratios, f"k_linattn_bwd_mfma/{kind}")


WIDE_BWD = [(dk, dv, h, w) for (dk, dv) in [(32, 64), (64, 128), (128, 64)] for (h, w) in [(5, 9), (7, 7)]] + [(64, 64) + _one_past(LW_TT)]


@pytest.mark.parametrize("kind", ["impulses", "dense"])
@pytest.mark.parametrize("dts", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", WIDE_BWD, ids=lambda c: f"2x{c[0]}x{c[1]}-{c[2]}x{c[3]}")
def test_linear_attention_wide_backward(case, dts, kind, ratios):
    dk, dv, h, w = case
    dtype, heads, n = DT[dts], 2, h * w
    if kind == "impulses":
        p = _impulses(ap.impulse_pairs(n, seed=n, edges=ap.edge5(n, LW_TT)), heads, dk, dv, h, w, dtype)
    else:
        p = _dense_bwd(heads, dk, dv, h, w, dtype)
    assert ops.linear_attention_wide_supported(p["qpre"].shape[0], n, heads * dk, heads * dv, heads, dtype)
    _check_backward(ops.LinearAttentionWideCoreFn, p, heads, dk, dv, h, w, dtype, "k_linattn_wide_bwd", ratios, f"k_linattn_wide_bwd/{kind}")
