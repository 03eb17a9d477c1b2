"""Probe inputs, a float64 reference and per-element bounds for the linear-attention kernels (rcx_attn.hip, rcx_attnw.hip, rcx_qkcore.hip).

Linear attention is an average over tokens: with dense zero-mean v one token's share of an output is about 1/n of a number that is itself small
next to pe, so a kernel that drops, doubles or misplaces ONE token stays inside any bar that is relative to the output.  The probes below make every
token count -- the output IS one token's v (or a constant), nothing cancels -- and the bounds are relative to the attention term itself.

The function (header of rcx_attnw.hip), on token-major tensors qpre, kpre (b, n, heads Dk), v, pe (b, n, heads Dv):

    q = elu(qpre) + 1,  k = elu(kpre) + 1,  kv = (1/n) k^T v,  kbar = mean_tokens(k),  u = q kv,  w = q . kbar + 1e-6,  out = u / w + pe

Probes (every value representable in the 16-bit type under test):
  live key      kpre = 1 on ONE token t* of the image (k = 2 exactly), -60 on the others (k = e^-60 = 9e-27); v[t*] ~ N(0, 1), v elsewhere N(0, 64^2)
                "poison".  Then out - pe = v[t*] S / (S + 1e-6) at every query token whatever q is: a dropped token is a relative error of 1, a pad
                token that enters the normaliser with k = 1 one of 1/3, k paired with a neighbour's v one of 1e4.
  unity         dense random qpre, kpre (the exp branch runs), v constant over the tokens of each (image, channel): out - pe = c S / (S + 1e-6).
                The numerator and the normaliser must see the same tokens with the same weights.
  two impulses  live key t* and dL/dout non-zero at ONE query token t0: gv[t*] = gout[t0] S / (S + 1e-6); gv elsewhere, gq and gk are 0 up to the
                1e-6 and the dead keys' 9e-27.  Every query token's share of dkv = q^T du and every key token's of dv shows on its own.
  gate channel  the same probes through the fused entry points that project kpre from d themselves: one channel g of d's key half holds +1 at t*
                and -1 elsewhere, W_k[:, g] = 32, every other key weight 0, b_k = -31: kpre = 1 and -63 exactly (bf16 operands, float32 sums).

What the probes do NOT vary freely: the live values are N(0, 1) pushed to at least 1/16 in magnitude, and pe is s times the expected attention term with
s in {-1/4, 1/4, 1/2, 1} (a small bias pack where the kernel computes pe).  Both keep a float32 output's own store rounding, which is relative to
|out| = |attention term + pe|, inside the bound's "+ 8", which is relative to the attention term alone.  So in every probe image pe is correlated with
the answer; an independent pe (N(0, 1), as in the existing tests) is checked by the dense cases only.

Bounds, per element, ref in float64 (nothing here is measured on the code under test):

    forward:   |got - ref| <= (R u16 + (n + Dk + 8 + extra) 2^-24) A + 1/2 ulp_out(max(|ref|, |got|)) + 1e-20
                 A = |ref - pe| for the probes (nothing cancels), A = M_u / w + |u| / w for dense inputs (M_u: u's sum over |v|)
    backward:  |got - ref| <= (R_b u16 + (n + Dk + Dv + 8 + extra) 2^-24) T + 1/2 ulp_out(...) + 1e-20

u16 = 2^-8 (bfloat16) / 2^-11 (float16) is the type the kernel rounds its matrix operands to, R / R_b how often its source does so on the way to an
element (ROUNDINGS below, with the lines); n + Dk (+ Dv) the float32 additions of the sums over tokens and channels; 8 the single roundings outside
them (the 1/n scalings, ksum / n, + 1e-6, the reciprocal or division, the final fma); `extra` what a kernel's source has beyond those eight.
The 1/2 ulp term is the store of a 16-bit output.  (elu1's __expf -- exp2 of the rounded product x log2(e), about 1 + |x| units of 2^-24 on q and k
where x <= 0 -- is NOT counted: if a kernel ever exceeds a bound by it, it goes into `extra` with its line, rcx_attn.hip:32.)
T is the float64 sum of the absolute values of the terms of the backward formulas (above k_linattn_bwd in rcx_attn.hip), an intermediate sum
entering through the sum of ITS terms' absolute values (as M_u does for u): for dq |du| |kv|^T + |dw| |kbar|, for dk (|v| |dkv|^T + |dkbar|) / n,
for dv |k| |dkv| / n, each times elu' where the chain has it.
"""
import math

import torch

from tests.grad64 import ulp16

U32 = 2.0 ** -24
U16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
FLOOR = 1e-20
DEAD = -60.0            # kpre of a dead key: k = e^-60 = 8.8e-27
POISON = 64.0           # standard deviation of v on the dead tokens
GATE_W, GATE_B = 32.0, -31.0            # the gate channel's key weight and bias: kpre = 32 (+-1) - 31 = 1 | -63

# How often a kernel's source rounds an operand to the 16-bit I/O type on the way to an output element (a conversion of a value that is already
# 16-bit -- v in the forward, v and gout's own load -- is exact and not counted), and its single float32 roundings beyond the eight of the bound.
# name: (R, extra, where)
ROUNDINGS = {
    # rcx_attn.hip
    "k_linattn_core":        (0, 0, "float32 throughout"),
    "k_linattn_core4":       (0, 0, "float32 throughout"),
    "k_linattn_mfma":        (3, 0, "k: A[j] = cvt(e) (:398); kv: KV0 / KV1 = cvt(t * s2) (:419-420); q: A0 / A1 = cvt(qq) (:450-451); v raw (:392)"),
    "k_linattn_bwd":         (0, 4, "float32 throughout; beyond the eight: g * u (:557), wsum * wsum (:568), dkv * s2 (:600), dkbar / n (:602)"),
    # k_linattn_bwd_mfma, per output (the longest chain of conversions into any term of the element's sum):
    #   dq = du kv^T + dw kbar: k (:682), kv as KVr (:718), du (:766-767); the dw term: k (:682), kv as KVa (:705-706), q (:744-745) -> 3
    #   dk = (v dkv^T + dkbar) / n: q (:806), du (:807), dkv as DKr (:846-847); v (:865-866) is exact; dkbar's dw as in dq -> 3
    #   dv = k dkv / n: q (:806), du (:807), dkv as DKa (:833-834), k (:865-866) -> 4
    "k_linattn_bwd_mfma":    ({"gq": 3, "gk": 3, "gv": 4}, 4, "see the lines above; beyond the eight as k_linattn_bwd: gg * uT (:754), wt * wt (:760), dk * s2 (:832), dkbar * s2 (:822)"),
    # rcx_attnw.hip
    "k_linattn_wide_fwd":    (0, 0, "float32 throughout"),
    "k_linattn_wide_bwd":    (0, 4, "float32 throughout; beyond the eight: g * u (:260), ws * ws (:270), dkv * inv_n (:297), dkbar * inv_n (:298)"),
    # rcx_qkcore.hip (operands bfloat16 whatever the I/O type): the projection's operands are d and the weight pack, both exact for probe data;
    # k: fa[j] = (__bf16)kk (:376 short, :703 / :850 long); kv: (__bf16)(kv * inv_n) (:387, :774, :889); q: (__bf16)qq (:182, :909); v = d exact
    "rcx_qkcore":            (3, 0, "k (:376 / :703 / :850), kv (:387 / :774 / :889), q (:182 / :909)"),
}


def elu1(x):
    """elu(x) + 1 without F.elu's expm1 + 1, which is exactly 0 in float64 at x = -60 where the kernels (and the function) have e^-60."""
    return torch.where(x > 0, x + 1, torch.exp(torch.clamp(x, max=0)))


def elu1_grad(x):
    return torch.where(x > 0, torch.ones_like(x), torch.exp(torch.clamp(x, max=0)))


def _split(x, heads):
    b, n, c = x.shape
    return x.reshape(b, n, heads, c // heads).permute(0, 2, 1, 3)          # b, heads, n, D


def _merge(x):
    b, h, n, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, h * d)


def core64(qpre, kpre, v, pe, heads, mutant=None):
    """The core in float64 -> dict of token-major (b, n, heads Dv) tensors out, u, w (broadcast over Dv), M_u.  `mutant` (tests only) is a
    function (q, k, v) (each b, heads, n, D) -> dict that may replace "kv" (b, heads, Dk, Dv) and "kbar" (b, heads, Dk) or add "u_add" (b, heads, 1 | n, Dv) to the
    numerator and "w_add" to the normaliser, see tests/test_attn_probe_cpu.py."""
    f = lambda t: t.detach().to(torch.float64) if not t.requires_grad else t
    qpre, kpre, v, pe = f(qpre), f(kpre), f(v), f(pe)
    n = qpre.shape[1]
    q, k, vv = _split(elu1(qpre), heads), _split(elu1(kpre), heads), _split(v, heads)
    kv = k.transpose(-1, -2) @ vv / n
    kva = k.transpose(-1, -2) @ vv.abs() / n
    kbar = k.mean(dim=2)
    m = {} if mutant is None else mutant(q, k, vv)
    kv, kbar = m.get("kv", kv), m.get("kbar", kbar)
    if "kv" in m:
        kva = kv.abs()
    u = q @ kv + m.get("u_add", 0.0)
    w = (q * kbar.unsqueeze(2)).sum(-1, keepdim=True) + 1e-6 + m.get("w_add", 0.0)
    out = _merge(u / w) + pe
    return {"out": out, "u": _merge(u), "w": _merge(w.expand_as(u)), "M_u": _merge(q @ kva)}


def grads64(qpre, kpre, v, gout, heads):
    """Float64 autograd of the core -> (ref, T): dicts gq, gk (b, n, heads Dk) and gv (b, n, heads Dv); T as in the module's header."""
    leaves = [t.detach().to(torch.float64).requires_grad_(True) for t in (qpre, kpre, v)]
    g = gout.detach().to(torch.float64)
    out = core64(leaves[0], leaves[1], leaves[2], torch.zeros_like(g), heads)["out"]
    gq, gk, gv = torch.autograd.grad(out, leaves, g)
    with torch.no_grad():
        qp, kp, vv = (t.detach() for t in leaves)
        n = qp.shape[1]
        q, k, va, ga = _split(elu1(qp), heads), _split(elu1(kp), heads), _split(vv.abs(), heads), _split(g.abs(), heads)
        kva = k.transpose(-1, -2) @ va / n                        # |kv|: b, heads, Dk, Dv
        kbar = k.mean(dim=2)                                      # b, heads, Dk
        w = (q * kbar.unsqueeze(2)).sum(-1, keepdim=True) + 1e-6   # b, heads, n, 1
        du = ga / w
        dw = (ga * (q @ kva)).sum(-1, keepdim=True) / (w * w)
        t_q = du @ kva.transpose(-1, -2) + dw * kbar.unsqueeze(2)
        dkv = q.transpose(-1, -2) @ du                            # b, heads, Dk, Dv
        dkbar = (q * dw).sum(dim=2)                               # b, heads, Dk
        t_k = (va @ dkv.transpose(-1, -2) + dkbar.unsqueeze(2)) / n
        t_v = k @ dkv / n
        T = {"gq": _merge(t_q) * elu1_grad(qp), "gk": _merge(t_k) * elu1_grad(kp), "gv": _merge(t_v)}
    return {"gq": gq, "gk": gk, "gv": gv}, T


def grads_by_formula(qpre, kpre, v, gout, heads, drop_query=None):
    """The backward formulas above k_linattn_bwd, term by term in float64 (equal to grads64's autograd; tests/test_attn_probe_cpu.py).  drop_query
    (tests only): a (B,) long tensor, the query token of each image that is left out of the dkv and dkbar sums."""
    qp, kp, vv, g = (t.detach().to(torch.float64) for t in (qpre, kpre, v, gout))
    n = qp.shape[1]
    q, k, vs, gs = _split(elu1(qp), heads), _split(elu1(kp), heads), _split(vv, heads), _split(g, heads)
    kv = k.transpose(-1, -2) @ vs / n
    kbar = k.mean(dim=2)
    u = q @ kv
    w = (q * kbar.unsqueeze(2)).sum(-1, keepdim=True) + 1e-6
    du = gs / w
    dw = -(gs * u).sum(-1, keepdim=True) / (w * w)
    dq = du @ kv.transpose(-1, -2) + dw * kbar.unsqueeze(2)
    keep = torch.ones(qp.shape[0], 1, n, 1, dtype=torch.float64, device=qp.device)
    if drop_query is not None:
        keep.scatter_(2, drop_query.view(-1, 1, 1, 1), 0.0)
    dkv = (q * keep).transpose(-1, -2) @ du
    dkbar = (q * keep * dw).sum(dim=2)
    dk = (vs @ dkv.transpose(-1, -2) + dkbar.unsqueeze(2)) / n
    dv = k @ dkv / n
    return {"gq": _merge(dq) * elu1_grad(qp), "gk": _merge(dk) * elu1_grad(kp), "gv": _merge(dv)}


def qk_project(d_tok, wqk, bqk):
    """The grouped 1x1 projection (groups = 2) in float64: d_tok (b, n, C), wqk (2C, C/2), bqk (2C) -> qpre, kpre (b, n, C)."""
    d_tok, wqk, bqk = (t.detach().to(torch.float64) for t in (d_tok, wqk, bqk))
    c = d_tok.shape[-1]
    qpre = d_tok[..., :c // 2] @ wqk[:c].t() + bqk[:c]
    kpre = d_tok[..., c // 2:] @ wqk[c:].t() + bqk[c:]
    return qpre, kpre


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------

def rel_bound(r, op_dtype, terms):
    """R u16 + terms 2^-24; op_dtype None (or float32) for an all-float32 kernel, whose R must be 0."""
    if r:
        return r * U16[op_dtype] + terms * U32
    return terms * U32


def elem_bound(got, ref, mag, rel, out_dtype):
    b = rel * mag + FLOOR
    if out_dtype in U16:
        b = b + 0.5 * ulp16(torch.maximum(ref.abs(), got.abs()), out_dtype)
    return b


def assert_within(got, ref, mag, rel, out_dtype, name):
    """Every element of got (any dtype, any device) against ref (float64) under elem_bound; -> the worst err / bound, where for a 16-bit output err
    and bound are both taken without the store's half ulp (with it every correctly rounded store would read 1; err <= bound is the same statement
    either way)."""
    g = got.detach().to(device=ref.device, dtype=torch.float64).reshape(ref.shape)
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    err = (g - ref).abs()
    bound = elem_bound(g, ref, mag, rel, out_dtype)
    core = (rel * mag + FLOOR).expand_as(ref)
    ratio = (err - (bound - core)).clamp(min=0) / core
    worst = float(ratio.max())
    if bool((err > bound).any()):
        i = int(ratio.reshape(-1).argmax())
        idx = []
        for s in reversed(ref.shape):
            idx.append(i % s)
            i //= s
        idx = tuple(reversed(idx))
        flat = lambda t: float(t[idx])
        raise AssertionError(
            f"{name} ({out_dtype}): {int((err > bound).sum())} of {err.numel()} elements outside the bound; worst at (image, token, channel) = {idx}: "
            f"got={flat(g):.9g} ref={flat(ref):.9g} |err|={flat(err):.3g} magnitude={flat(mag.expand_as(ref)):.3g} bound={flat(bound):.3g} "
            f"(rel={rel:.3g}), err / bound = {worst:.3g}")
    return worst


def fwd_rel(kernel, n, dk, op_dtype):
    r, extra, _ = ROUNDINGS[kernel]
    return rel_bound(r, op_dtype, n + dk + 8 + extra)


def bwd_rel(kernel, which, n, dk, dv, op_dtype):
    r, extra, _ = ROUNDINGS[kernel]
    if isinstance(r, dict):
        r = r[which]
    return rel_bound(r, op_dtype, n + dk + dv + 8 + extra)


# ---- token lists ----------------------------------------------------------------------------------------------------------------------------

def token_list(n, steps=(16, 32), waves=4, every=None, seed=0, n_random=32):
    """The tokens a probe makes live, one image each.  every=True (default for n <= 1024): all of them.  Otherwise the edges -- 0, 15, 16, 31, 32,
    63, 64, 127, 128, n-33, n-32, n-17, n-16, n-2, n-1 --, the first and last token of each wave's first and last step when the tokens are dealt
    over `waves` waves in steps of `steps`, and n_random seeded random ones.  Sorted, without repeats."""
    if every is None:
        every = n <= 1024
    if every:
        return list(range(n))
    toks = {0, 15, 16, 31, 32, 63, 64, 127, 128, n - 33, n - 32, n - 17, n - 16, n - 2, n - 1}
    for step in steps:
        for w in range(waves):
            first = step * w
            if first >= n:
                continue
            last = first + ((n - 1 - first) // (step * waves)) * step * waves
            for t0 in (first, last):
                toks.update((t0, min(t0 + step - 1, n - 1)))
    g = torch.Generator().manual_seed(seed)
    toks.update(int(t) for t in torch.randint(0, n, (n_random,), generator=g))
    return sorted(t for t in toks if 0 <= t < n)


# ---- probe inputs (made on `device` from a seeded generator of that device) -----------------------------------------------------------------

def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _rn(g, shape, dtype, scale=1.0):
    """N(0, scale^2) rounded to dtype (returned in dtype)."""
    return (torch.randn(shape, generator=g, device=g.device, dtype=torch.float32) * scale).to(dtype)


def _away(g, shape, dtype, scale=1.0):
    """N(0, scale^2) with magnitudes of at least scale / 16, rounded to dtype: values the bounds are relative to (a float32 output's own rounding is
    covered by the bound's 8 only while pe stays within two orders of the attention term)."""
    x = torch.randn(shape, generator=g, device=g.device, dtype=torch.float32) * scale
    x = torch.where(x.abs() < scale / 16, torch.copysign(torch.full_like(x, scale / 16), x), x)
    return x.to(dtype)


def _pe_like(g, a, dtype):
    """pe = s a with s in {-1/4, 1/4, 1/2, 1} per element: 16-bit representable and of the attention term's own size."""
    s = torch.tensor([-0.25, 0.25, 0.5, 1.0], device=a.device)[torch.randint(0, 4, a.shape, generator=g, device=a.device)]
    return (a.to(torch.float32) * s).to(dtype)


def live_key(tokens, n, heads, dk, dv, dtype, device="cpu", seed=0, per_head=False):
    """One image per entry of `tokens`.  -> dict qpre, kpre (B, n, heads dk), v, pe (B, n, heads dv) in dtype, live (B, heads) long: the live token
    of each (image, head) (per_head: head j of image i lives at tokens[(i + 7 j) % B])."""
    g = _gen(device, seed)
    bsz = len(tokens)
    tok = torch.tensor(tokens, device=device, dtype=torch.long)
    live = torch.stack([tok[(torch.arange(bsz, device=device) + 7 * j * int(per_head)) % bsz] for j in range(heads)], dim=1)      # B, heads
    qpre = _rn(g, (bsz, n, heads * dk), dtype, 0.7)
    is_live = torch.zeros(bsz, heads, n, dtype=torch.bool, device=device).scatter_(2, live.unsqueeze(-1), True).permute(0, 2, 1)  # B, n, heads
    kpre = torch.where(is_live.repeat_interleave(dk, dim=2), 1.0, DEAD).to(dtype)
    lv = is_live.repeat_interleave(dv, dim=2)
    v = torch.where(lv, _away(g, (bsz, n, heads * dv), dtype).float(), _rn(g, (bsz, n, heads * dv), dtype, POISON).float()).to(dtype)
    a = (v.float() * lv).sum(dim=1, keepdim=True).expand(bsz, n, heads * dv)          # v[t*] of the channel's head, at every token
    return {"qpre": qpre, "kpre": kpre, "v": v, "pe": _pe_like(g, a, dtype), "live": live}


def unity(bsz, n, heads, dk, dv, dtype, device="cpu", seed=0):
    """Dense qpre, kpre; v constant over the tokens of each (image, channel)."""
    g = _gen(device, seed)
    qpre, kpre = _rn(g, (bsz, n, heads * dk), dtype, 0.7), _rn(g, (bsz, n, heads * dk), dtype, 0.7)
    v = _away(g, (bsz, 1, heads * dv), dtype).expand(bsz, n, heads * dv).contiguous()
    return {"qpre": qpre, "kpre": kpre, "v": v, "pe": _pe_like(g, v, dtype)}


def dense(bsz, n, heads, dk, dv, dtype, device="cpu", seed=0):
    """The existing tests' kind of input: everything dense and random."""
    g = _gen(device, seed)
    return {"qpre": _rn(g, (bsz, n, heads * dk), dtype, 0.7), "kpre": _rn(g, (bsz, n, heads * dk), dtype, 0.7),
            "v": _rn(g, (bsz, n, heads * dv), dtype), "pe": _rn(g, (bsz, n, heads * dv), dtype), "gout": _rn(g, (bsz, n, heads * dv), dtype, 0.7)}


def two_impulses(pairs, n, heads, dk, dv, dtype, device="cpu", seed=0):
    """One image per (t*, t0) of `pairs`: the live-key probe at t* and gout non-zero at query token t0 only.  Adds gout and query (B,) long."""
    p = live_key([a for a, _ in pairs], n, heads, dk, dv, dtype, device, seed)
    g = _gen(device, seed + 1)
    bsz = len(pairs)
    t0 = torch.tensor([b for _, b in pairs], device=device, dtype=torch.long)
    at = torch.zeros(bsz, n, 1, dtype=torch.bool, device=device).scatter_(1, t0.view(bsz, 1, 1), True)
    p["gout"] = torch.where(at, _away(g, (bsz, n, heads * dv), dtype).float(), 0.0).to(dtype)
    p["query"] = t0
    return p


def impulse_pairs(n, seed=0, every=None, edges=None, n_random=32):
    """(t*, t0) pairs.  edges: a token list -> its square plus n_random random pairs.  Otherwise every t* with a random t0 and every t0 with a random
    t* (the tokens of token_list(n, every=every))."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: int(torch.randint(0, n, (1,), generator=g))
    if edges is not None:
        return [(a, b) for a in edges for b in edges] + [(rnd(), rnd()) for _ in range(n_random)]
    toks = token_list(n, every=every, seed=seed)
    return [(t, rnd()) for t in toks] + [(rnd(), t) for t in toks]


def step_edges(n, steps=(16, 32)):
    """The first and last token of the first steps of a kernel that walks the tokens in `steps`, and the last two tokens: for the small planes of
    the matrix-core kernels (0, 15, 16, 31, 32, 47, 48, 63, 64, n - 2, n - 1 for steps of 16 and 32)."""
    toks = {0, n - 2, n - 1}
    for s in steps:
        for j in range(1, 64 // s + 1):
            toks.update((j * s - 1, j * s))
    return sorted(t for t in toks if 0 <= t < n)


def kernel_constant(source, name):
    """An integer `constexpr int NAME = value;` read from a kernel source under recnext_amd/csrc (the tests take tile and step sizes from the kernels,
    so that a plane "one past a tile" stays one when the tile changes)."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recnext_amd", "csrc", source)
    with open(path) as f:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", f.read())
    assert m, f"{name} not found in {source}"
    return int(m.group(1))


def edge5(n, tile):
    """Five tokens around the kernel's token tile: first, last of the first tile, first of the second (if any), the middle, the last."""
    return sorted({0, min(tile, n) - 1, min(tile, n - 1), n // 2, n - 1})


# ---- the fused entry points: the probes through the projection ------------------------------------------------------------------------------

def gate_live_key(tokens, n, heads, d, device="cpu", seed=0, dtype=torch.bfloat16):
    """The live-key probe for recattn_qkcore: d_tok (B, n, C = heads d) float32 of bfloat16-representable values (`dtype`: a second 16-bit type the values
    must also fit, for the entry that takes x), wqk (2C, C/2) bfloat16, bqk (2C) float32.  The gate channel is the LAST channel of d (key half); v = d,
    so on it the expected attention term is +1.  b_pe (C) float32; the pe taps are the caller's zeros."""
    g = _gen(device, seed)
    bsz, c = len(tokens), heads * d
    r16 = lambda t: t.to(torch.bfloat16).to(dtype).to(torch.float32)
    tok = torch.tensor(tokens, device=device, dtype=torch.long)
    is_live = torch.zeros(bsz, n, 1, dtype=torch.bool, device=device).scatter_(1, tok.view(bsz, 1, 1), True)
    dt = torch.where(is_live, r16(_away(g, (bsz, n, c), torch.bfloat16).float()), r16(_rn(g, (bsz, n, c), torch.bfloat16, POISON).float()))
    dt[..., c - 1] = torch.where(is_live[..., 0], 1.0, -1.0)
    wqk = torch.zeros(2 * c, c // 2, device=device)
    wqk[:c] = torch.randn(c, c // 2, generator=g, device=device) * (0.7 / (POISON * math.sqrt(c / 2)))
    wqk[c:, c // 2 - 1] = GATE_W
    bqk = torch.cat([torch.randn(c, generator=g, device=device) * 0.3, torch.full((c,), GATE_B, device=device)])
    b_pe = _away(g, (c,), torch.bfloat16, 0.25).float()
    return {"d": dt, "wqk": wqk.to(torch.bfloat16), "bqk": bqk, "b_pe": b_pe, "live": tok}


def gate_unity(bsz, n, heads, d, device="cpu", seed=0):
    """The unity probe for recattn_qkcore: d constant over the tokens of each (image, channel), random projection (no gate)."""
    g = _gen(device, seed)
    c = heads * d
    dt = _away(g, (bsz, 1, c), torch.bfloat16).float().expand(bsz, n, c).contiguous()
    wqk = (torch.randn(2 * c, c // 2, generator=g, device=device) * (0.7 / math.sqrt(c / 2))).to(torch.bfloat16)
    bqk = torch.randn(2 * c, generator=g, device=device) * 0.3
    return {"d": dt, "wqk": wqk, "bqk": bqk, "b_pe": _away(g, (c,), torch.bfloat16, 0.25).float()}


def gate_reference(p, heads):
    """core64 of a gate probe (pe = the bias alone: zero taps) -> (core64's dict, pe)."""
    qpre, kpre = qk_project(p["d"], p["wqk"], p["bqk"])
    pe = p["b_pe"].to(torch.float64).expand_as(p["d"])
    return core64(qpre, kpre, p["d"], pe, heads), pe
