"""CPU: the attention probes of tests/attn_probe.py are honest -- the float64 reference is the function the other references compute, the closed
forms hold for it, a correct 16-bit-operand kernel fits inside the bounds, and every single-token mutant of the reference falls outside them
on at least one probe image (while the token mutants pass the flat 1e-2 + 1e-2 |ref| bar on dense inputs, which is why the probes exist)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recconv_np
from tests import attn_probe as ap
from tests import ls_eager

BF = torch.bfloat16
PLANES = [16, 45, 49, 513, 784]


def _tokens(n):
    return ap.token_list(n, every=n <= 64)


# ---- 1. the reference is the function -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [1, 2])
def test_reference_agrees_with_the_numpy_oracle(variant):
    g = torch.Generator().manual_seed(variant)
    b, c, h, w, heads = 2, 24, 5, 7, 2
    x = torch.randn(b, c, h, w, generator=g, dtype=torch.float64)
    wqk = torch.randn(2 * c, c // 2, generator=g, dtype=torch.float64) * 0.3
    bqk = torch.randn(2 * c, generator=g, dtype=torch.float64) * 0.3
    wpe = torch.randn(c, 1, 3, 3, generator=g, dtype=torch.float64) * 0.3
    bpe = torch.randn(c, generator=g, dtype=torch.float64) * 0.3
    want = recconv_np.linear_attention(x.numpy(), wqk.numpy().reshape(2 * c, c // 2, 1, 1), bqk.numpy(), wpe.numpy(), bpe.numpy(), heads, variant)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(b, h * w, c)
    qpre, kpre = ap.qk_project(tok(x), wqk, bqk)
    got = ap.core64(qpre, kpre, tok(x), tok(F.conv2d(x, wpe, bpe, padding=1, groups=c)), heads)["out"]
    np.testing.assert_allclose(got.numpy(), tok(torch.from_numpy(want)).numpy(), rtol=0, atol=1e-9)


@pytest.mark.parametrize("dk,dv", [(12, 12), (8, 20)])
def test_reference_agrees_with_the_eager_restatements(dk, dv):
    p = ap.dense(3, 35, 2, dk, dv, torch.float64, seed=dk)
    got = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], 2)["out"]
    heads_first = lambda t, d: t.reshape(3, 35, 2, d).permute(0, 2, 3, 1)                   # b, heads, d, n
    att = ls_eager._attend(heads_first(ap.elu1(p["qpre"]), dk), heads_first(ap.elu1(p["kpre"]), dk), heads_first(p["v"], dv), 35 ** -0.5)
    assert float((att.permute(0, 2, 1, 3).reshape(3, 35, 2 * dv) + p["pe"] - got).abs().max()) <= 1e-9
    if dk == dv:
        from tests.test_backward_gpu import _la_reference
        assert float((_la_reference(p["qpre"], p["kpre"], p["v"], p["pe"], 2) - got).abs().max()) <= 1e-9


def test_formula_gradients_are_autograd():
    p = ap.dense(2, 21, 2, 8, 12, torch.float64, seed=5)
    ref, T = ap.grads64(p["qpre"], p["kpre"], p["v"], p["gout"], 2)
    by = ap.grads_by_formula(p["qpre"], p["kpre"], p["v"], p["gout"], 2)
    for name in ("gq", "gk", "gv"):
        assert float((ref[name] - by[name]).abs().max()) <= 1e-12
        assert bool((ref[name].abs() <= T[name] * (1 + 1e-12)).all()), "T bounds the gradient it is the absolute-value sum of"


# ---- 2. the closed forms --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("n", PLANES)
def test_live_key_closed_form(n, heads):
    toks = _tokens(n)
    p = ap.live_key(toks, n, heads, 32, 12, BF, seed=n, per_head=True)
    r = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], heads)
    vd = p["v"].double().reshape(len(toks), n, heads, 12)
    want = torch.stack([vd[torch.arange(len(toks)), p["live"][:, j], j] for j in range(heads)], dim=1).reshape(len(toks), 1, heads * 12)
    a = r["out"] - p["pe"].double()
    assert float(((a - want).abs() / want.abs()).max()) <= 7e-5                            # whatever q is: 1e-6 / S at 32-wide heads
    s = (2.0 / n) * ap.elu1(p["qpre"].double()).reshape(len(toks), n, heads, 32).sum(-1)    # S = q . kbar, kbar = 2 / n on every channel
    exact = want.reshape(len(toks), 1, heads, 12) * (s / (s + 1e-6)).unsqueeze(-1)
    assert float(((a - exact.reshape(a.shape)).abs() / want.abs()).max()) <= 1e-9


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("n", PLANES)
def test_unity_closed_form(n, heads):
    p = ap.unity(3, n, heads, 32, 12, BF, seed=n)
    r = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], heads)
    a = r["out"] - p["pe"].double()
    assert float(((a - p["v"].double()).abs() / p["v"].double().abs()).max()) <= 7e-5


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("dk,dv", [(32, 32), (64, 128)])
@pytest.mark.parametrize("n", PLANES)
def test_two_impulses_closed_form(n, dk, dv, heads):
    """With P = gout[t0] . v[t*] per head, S = q[t0] . kbar = (2 / n) sum q[t0] and w = S + 1e-6, exactly (up to the dead keys' e^-60):
        gv[t*] = gout[t0] S / w,   gq[t0] = elu'(qpre[t0]) (2 / n) P 1e-6 / w^2,   gk[t*] = q[t0] P 1e-6 / (n w^2),   everything else 0.
    The deviation from gv[t*] = gout[t0], gq = gk = 0 is 1e-6 / S and grows with n: within 1e-5 (relative) and 4e-6 up to n = 513; at n = 784 with 32-wide
    heads it is 1.5e-5, max |gq| 7.1e-6 and max |gk| 7.9e-6, so there only the exact forms are asserted."""
    pairs = ap.impulse_pairs(n, seed=n, edges=ap.edge5(n, 32), n_random=8)
    p = ap.two_impulses(pairs, n, heads, dk, dv, BF, seed=n)
    ref, _ = ap.grads64(p["qpre"], p["kpre"], p["v"], p["gout"], heads)
    bsz = len(pairs)
    i = torch.arange(bsz)
    live, query = p["live"][:, 0], p["query"]
    g0 = p["gout"].double()[i, query].reshape(bsz, heads, dv)
    vs = p["v"].double()[i, live].reshape(bsz, heads, dv)
    qp0 = p["qpre"].double()[i, query].reshape(bsz, heads, dk)
    q0 = ap.elu1(qp0)
    big_s = (2.0 / n) * q0.sum(-1, keepdim=True)                                           # B, heads, 1
    w = big_s + 1e-6
    dot = (g0 * vs).sum(-1, keepdim=True)
    gv_x = torch.zeros_like(ref["gv"])
    gv_x[i, live] = (g0 * big_s / w).reshape(bsz, -1)
    gq_x = torch.zeros_like(ref["gq"])
    gq_x[i, query] = (ap.elu1_grad(qp0) * (2.0 / n) * dot * 1e-6 / (w * w)).reshape(bsz, -1)
    gk_x = torch.zeros_like(ref["gk"])
    gk_x[i, live] = (q0 * dot * 1e-6 / (n * w * w)).reshape(bsz, -1)
    # gq and gk are what float64 leaves of two terms of size |P| / (n w) that cancel to 1e-6 / w of themselves: allow 1e-13 of those terms
    # (a few hundred float64 roundings over the Dv products), still under a hundredth of the values being checked
    cancel = 1e-13 * dv * float(g0.abs().max()) * float(vs.abs().max()) + 1e-20
    for name, exact, tol in (("gv", gv_x, 1e-9 * float(gv_x.abs().max())), ("gq", gq_x, cancel), ("gk", gk_x, cancel)):
        err = (ref[name] - exact).abs()
        assert float(err.max()) <= tol, f"{name}: {float(err.max()):.3g} > {tol:.3g}"
        assert tol <= 1e-2 * float(exact.abs().max()), "the tolerance must stay far below the closed form's own values"
    if n <= 513:                                                                           # the looser statement, where it holds
        assert float(((ref["gv"][i, live].reshape(bsz, heads, dv) - g0).abs() / g0.abs()).max()) <= 1e-5
        assert float(ref["gq"].abs().max()) <= 4e-6 and float(ref["gk"].abs().max()) <= 4e-6


# ---- 3. a correct kernel with 16-bit operands fits ------------------------------------------------------------------------------------------

def _emulate_bf16(p, heads):
    """The matrix-core kernel's arithmetic in torch: q, k and kv (1/n) rounded to bfloat16, float32 sums, the normaliser from the unrounded q."""
    f = lambda t: t.float()
    n = p["qpre"].shape[1]
    q, k, v = ap._split(ap.elu1(f(p["qpre"])), heads), ap._split(ap.elu1(f(p["kpre"])), heads), ap._split(f(p["v"]), heads)
    r = lambda t: t.to(BF).float()
    kv = r((r(k).transpose(-1, -2) @ v) * (1.0 / n))
    w = (q * k.mean(dim=2).unsqueeze(2)).sum(-1, keepdim=True) + 1e-6
    return (ap._merge(r(q) @ kv / w) + f(p["pe"])).to(BF)


@pytest.mark.parametrize("n", [513, 784])
@pytest.mark.parametrize("probe", ["live", "unity"])
def test_bf16_operand_emulation_is_inside_the_bound(probe, n, record_property):
    p = ap.live_key(ap.token_list(n, every=False), n, 2, 32, 32, BF, seed=n) if probe == "live" else ap.unity(4, n, 2, 32, 32, BF, seed=n)
    ref = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], 2)["out"]
    a = (ref - p["pe"].double()).abs()
    got = _emulate_bf16(p, 2)
    rel = ap.fwd_rel("k_linattn_mfma", n, 32, BF)
    record_property("worst_ratio", ap.assert_within(got, ref, a, rel, BF, f"emulation {probe} n={n}"))
    # the part of the error beyond the store's half ulp, in units of 2^-8 a: the bound's R = 3 is reachable (measured 1.34) but not exceeded
    err = ((got.double() - ref).abs() - 0.5 * ap.ulp16(torch.maximum(ref.abs(), got.double().abs()), BF)).clamp(min=0) / (2.0 ** -8 * a)
    record_property("worst_units_of_u16", float(err.max()))
    assert float(err.max()) < 3.0


# ---- 4. every mutant is caught --------------------------------------------------------------------------------------------------------------

def _drop(tok, what):
    def m(q, k, v):
        n = q.shape[2]
        i = torch.arange(q.shape[0])
        kt, vt = k[i, :, tok], v[i, :, tok]                                                # b, heads, D
        out = {}
        if "kv" in what:
            out["kv"] = k.transpose(-1, -2) @ v / n - kt.unsqueeze(-1) * vt.unsqueeze(-2) / n
        if "kbar" in what:
            out["kbar"] = k.mean(dim=2) - kt / n
        return out
    return m


def _pad(count):
    """`count(n)` pad tokens with kpre = 0, v = 0: k = elu(0) + 1 = 1 enters the normaliser."""
    return lambda q, k, v: {"kbar": k.mean(dim=2) + count(q.shape[2]) / q.shape[2]}


TOKEN_MUTANTS = {                                                                          # name -> (mutant factory (tok) , is the identity at n)
    "token dropped from kv and kbar": (lambda tok: _drop(tok, ("kv", "kbar")), lambda n: False),
    "token dropped from kv": (lambda tok: _drop(tok, ("kv",)), lambda n: False),
    "token dropped from kbar": (lambda tok: _drop(tok, ("kbar",)), lambda n: False),
    "one pad token in the normaliser": (lambda tok: _pad(lambda n: 1), lambda n: False),
    "pad tokens to a multiple of 16": (lambda tok: _pad(lambda n: -n % 16), lambda n: n % 16 == 0),
    "pad tokens to a multiple of 32": (lambda tok: _pad(lambda n: -n % 32), lambda n: n % 32 == 0),
}
OTHER_MUTANTS = {
    "k paired with the next token's v": lambda q, k, v: {"kv": k.transpose(-1, -2) @ torch.roll(v, -1, dims=2) / q.shape[2]},
    "two heads' kv swapped": lambda q, k, v: {"kv": (k.transpose(-1, -2) @ v / q.shape[2]).flip(1)},
    "kv transposed": lambda q, k, v: {"kv": (k.transpose(-1, -2) @ v / q.shape[2]).transpose(-1, -2)},
    # a padded channel with q = k = 1 on every token: kv's padded row is mean_tokens(v), which q = 1 adds to the numerator, and kbar's padded entry is 1
    "a padded key channel with q = k = 1": lambda q, k, v: {"u_add": v.mean(dim=2, keepdim=True), "w_add": 1.0},
}


def _probe_ratios(n, d, mutant_of):
    """Worst err / bound per probe (live key per image, unity) of a mutant of the reference, under the LOOSEST forward bound any kernel has
    (three bfloat16 operand roundings, a bfloat16 output).  Every token of the plane gets its probe image up to n = 513; n = 784 uses the edge list
    of attn_probe.token_list (the edges of the 16- and 32-token steps of four waves plus 32 random tokens)."""
    toks = ap.token_list(n, every=n <= 600)
    live = ap.live_key(toks, n, 2, d, d, BF, seed=n)
    uni = ap.unity(len(toks), n, 2, d, d, BF, seed=n + 1)
    res = {}
    for name, p, tok in (("live key", live, live["live"][:, 0]), ("unity", uni, torch.tensor(toks))):
        ref = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], 2)["out"]
        got = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], 2, mutant=mutant_of(tok))["out"]
        a = (ref - p["pe"].double()).abs()
        rel = ap.fwd_rel("k_linattn_mfma", n, d, BF)
        res[name] = ((got - ref).abs() / ap.elem_bound(got, ref, a, rel, BF)).amax(dim=(1, 2))          # per probe image
    return res


@pytest.mark.parametrize("n", [45, 49, 513, 784])
def test_every_forward_mutant_is_outside_the_probe_bounds(n, record_property):
    report = {}
    for name, (make, identity) in TOKEN_MUTANTS.items():
        if identity(n):
            continue
        res = _probe_ratios(n, 8, make)
        best = max(res, key=lambda k: float(res[k].max()))
        report[name] = (best, float(res[best].max()))
        # a token mutant is about ONE token: the probe image whose live key that token is must catch it, whichever token it is
        if "dropped" in name:
            assert bool((res["live key"] > 1).all()), f"{name}: {int((res['live key'] <= 1).sum())} tokens escape the live-key probe at n={n}"
    for name, mutant in OTHER_MUTANTS.items():
        res = _probe_ratios(n, 8, lambda tok: mutant)
        best = max(res, key=lambda k: float(res[k].max()))
        report[name] = (best, float(res[best].max()))
    for name, (probe, factor) in report.items():
        print(f"n={n}: {name}: caught by the {probe} probe, err / bound = {factor:.3g}")
        record_property(name, f"{probe}: {factor:.3g}")
        assert factor > 1.0, f"{name} passes every probe at n={n} (worst err / bound {factor:.3g}, {probe})"


@pytest.mark.parametrize("n", [45, 49, 513])
def test_a_dropped_query_token_is_outside_the_backward_bounds(n, record_property):
    """Any single query token left out of the dkv / dkbar sums: the pair whose impulse sits on that token loses gv[t*] altogether.  Every token
    of the plane is tried."""
    toks = list(range(n))
    g = torch.Generator().manual_seed(n)
    pairs = [(int(torch.randint(0, n, (1,), generator=g)), t) for t in toks]
    p = ap.two_impulses(pairs, n, 2, 8, 8, BF, seed=n)
    ref, T = ap.grads64(p["qpre"], p["kpre"], p["v"], p["gout"], 2)
    got = ap.grads_by_formula(p["qpre"], p["kpre"], p["v"], p["gout"], 2, drop_query=p["query"])
    rel = ap.bwd_rel("k_linattn_bwd_mfma", "gv", n, 8, 8, BF)
    ratio = ((got["gv"] - ref["gv"]).abs() / ap.elem_bound(got["gv"], ref["gv"], T["gv"], rel, BF)).amax(dim=(1, 2))
    print(f"n={n}: query token dropped from dkv / dkbar: caught by two impulses, err / bound >= {float(ratio.min()):.3g} on every pair")
    record_property("least_ratio", float(ratio.min()))
    assert bool((ratio > 1).all())
    same = ap.grads_by_formula(p["qpre"], p["kpre"], p["v"], p["gout"], 2)
    for name in ("gq", "gk", "gv"):
        r = ap.bwd_rel("k_linattn_bwd", name, n, 8, 8, None)
        ap.assert_within(same[name], ref[name], T[name], r, torch.float32, f"the unmutated formulas, {name}")


@pytest.mark.parametrize("case", [(2, 80, 2, 28, 28), (1, 72, 2, 56, 56)], ids=lambda c: "x".join(map(str, c)))
def test_token_mutants_pass_the_flat_bar_on_dense_inputs(case, record_property):
    """The reason the probes exist: on the dense inputs of the large existing cases the six token mutants stay inside 1e-2 + 1e-2 |ref|."""
    b, c, heads, h, w = case
    n, d = h * w, c // heads
    p = ap.dense(b, n, heads, d, d, BF, seed=c)
    ref = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], heads)["out"]
    last = torch.full((b,), n - 1, dtype=torch.long)
    for name, (make, identity) in TOKEN_MUTANTS.items():
        got = ap.core64(p["qpre"], p["kpre"], p["v"], p["pe"], heads, mutant=make(last))["out"]
        worst = float(((got - ref).abs() / (1e-2 + 1e-2 * ref.abs())).max())
        record_property(name, round(worst, 4))
        assert worst < 1.0, f"{name}: err / tol = {worst:.3g}"


def test_token_lists():
    assert ap.token_list(49) == list(range(49))
    big = ap.token_list(3136)
    assert {0, 15, 16, 31, 32, 63, 64, 127, 128, 3103, 3104, 3119, 3120, 3134, 3135} <= set(big) and len(big) < 120
    for step in (16, 32):                                                                  # each of the four waves' first and last step
        for wv in range(4):
            starts = list(range(step * wv, 3136, 4 * step))
            assert {starts[0], starts[0] + step - 1, starts[-1], min(starts[-1] + step - 1, 3135)} <= set(big)
    assert ap.token_list(784, every=False) == sorted(set(ap.token_list(784, every=False))) and max(ap.token_list(513, every=False)) == 512
