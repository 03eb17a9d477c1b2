"""Float64 reference and per-element bounds for RepVGGDW on batch statistics as one operator (rcx_repdw_train_*; lsnet/model/recattn.py:8-15).
tests/test_repdw_cpu.py holds the operator chain on ATen in float32 on the CPU to them, tests/test_repdw_gpu.py the HIP kernels on the GPU.

The reference evaluates the operator's formulas (include/recnext_amd.h) in float64 on the very values the kernel sees: 16-bit inputs widened exactly,
eps and momentum as the float32 they are passed as.  The backward's reference takes the saved float32 statistics (mean x, var x, mean u, ia) as given
constants, as tests/bn64.py's does.  Every output comes as (ref, mag) and is checked with tests/grad64.py's assert_grad_close at its K = 24 units of
u32 = 2^-24 (never raised: an excess is a kernel bug).  mag follows bn64 / grad64: every sum and product over absolute values, and every quantity that
passes through a normalisation carries bn64's condition factor (1 + a r), a the channel's mean magnitude and r its inverse standard deviation.  With
U = sum |w3| |x| + |b3| the magnitude of u, au = mean U, ax = mean |x|, V = |w1| |x| + |b1| the magnitude of v = w1 x + b1, av = mean V,
uhat = (u - mean u) ia, vhat = w1 (x - mean x) ib, ka = 1 + au ia, kb = 1 + av ib:

    mean x   ax                 var x   vx + ax sqrt(vx)             mean u   au                ia   ia ka
    lk running mean / var       (1 - m) |old| + m au                 (1 - m) old + m var_u R / (R - 1) ka
    sk running mean / var       (1 - m) |old| + m av                 (1 - m) old + m w1^2 var_x R / (R - 1) kb
    r        |gamma_a| [ia (U + au) + |uhat| ka] + |beta_a| + |gamma_b| [ib (V + av) + |vhat| kb] + |beta_b| + |x|
    mu = (U + au) ia + |uhat|,  mv = ((V + av) ib + |vhat|) kb        (ib is formed from var x at every use, so the sk terms keep the factor)
    gbeta_a, gbeta_b   sum |g|          ggamma_a   sum |g| mu          ggamma_b   sum |g| mv
    |gu| = |gamma_a| ia (|g| + sum |g| / R + |uhat| sum(|g| mu) / R + mu |Su| / R)         Su = sum g uhat
    |gv| = |gamma_b| ib (|g| + sum |g| / R + |vhat| sum(|g| mv) / R + mv |Sv| / R) kb      Sv = sum g vhat
    gw3[d]   sum_p |gu|(p) |x|(p + d)          gb3   sum |gu|  (ref: the float64 sum gu)          gw1   sum |gv| |x|          gb1   sum |gv|  (ref: sum gv)
    gx       sum_d |w3[d]| |gu|(q - d) + |w1| |gv| + |g|

gw1's reference is the closed form gamma_b eps_b ib^3 Sx; an operator that sums gv x instead (autograd of the chain) differs from it by what the
constants' own rounding leaves of the cancellation, which sum |gv| |x| covers.  Half an ulp of the output type comes on top for a 16-bit output."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import bn64, grad64

EXTRA_SHAPES = [(1, 16, 2, 3), (2, 16, 1, 6), (2, 16, 6, 1), (2, 384, 7, 7)]
SHAPES = bn64.SHAPES + EXTRA_SHAPES
MOM_A, EPS_A, MOM_B, EPS_B = 0.1, 1e-5, 0.2, 1e-3
PARAMS = ("w3", "b3", "gamma_a", "beta_a", "w1", "b1", "gamma_b", "beta_b")
RUNNING = ("lk_running_mean", "lk_running_var", "sk_running_mean", "sk_running_var")
STATS = ("mean_x", "var_x", "mean_u", "invstd_u")
GRADS = ("gw3", "gb3", "ggamma_a", "gbeta_a", "gw1", "gb1", "ggamma_b", "gbeta_b")

_CASES = {}


def case(shape, dtype, dist):
    """bn64.case's x and gy (the latter is g = dL/dr) and, from a seeded generator, the float32 parameters and running buffers: one channel's w1 is 0
    and, where there is a second channel, one is negative."""
    key = (shape, dtype, dist)
    if key not in _CASES:
        b = bn64.case(shape, dtype, dist)
        c = shape[1]
        gen = torch.Generator().manual_seed(1000 + sum(shape) * 7 + bn64.DISTS.index(dist))
        rn = lambda *s: torch.randn(*s, generator=gen)
        d = dict(x=b["x"], g=b["gy"], w3=rn(c, 1, 3, 3) * 0.3, b3=rn(c) * 0.2, gamma_a=rn(c) * 0.5 + 1.0, beta_a=rn(c) * 0.3, w1=rn(c, 1, 1, 1) * 0.5 + 1.0,
                 b1=rn(c) * 0.2, gamma_b=rn(c) * 0.5 + 1.0, beta_b=rn(c) * 0.3, lk_running_mean=rn(c) * 0.2, lk_running_var=torch.rand(c, generator=gen) + 0.5,
                 sk_running_mean=rn(c) * 0.2, sk_running_var=torch.rand(c, generator=gen) + 0.5)
        d["w1"][0] = 0.0
        if c > 1:
            d["w1"][c - 1] = -0.75
        _CASES[key] = d
    return _CASES[key]


def _f32(v):
    return float(np.float32(v))


def _d(t):
    return t.detach().double().cpu()


def _conv(x, w3, b3):
    return F.conv2d(x, w3, b3, padding=1, groups=x.shape[1])


def _common(x, p):
    """float64 pieces both references share: x, u, their magnitudes (R x C) and channel means."""
    x4 = _d(x)
    w3, b3, w1, b1 = _d(p["w3"]), _d(p["b3"]), _d(p["w1"]).flatten(), _d(p["b1"])
    u4, U4 = _conv(x4, w3, b3), _conv(x4.abs(), w3.abs(), b3.abs())
    x2, u2, U2 = bn64.rows(x4), bn64.rows(u4), bn64.rows(U4)
    V2 = w1.abs() * x2.abs() + b1.abs()
    return dict(x4=x4, x2=x2, u2=u2, U2=U2, V2=V2, ax=x2.abs().mean(0), au=U2.mean(0), av=V2.mean(0), w3=w3, w1=w1, b1=b1)


def forward_ref(x, p, running=None, mom_a=MOM_A, eps_a=EPS_A, mom_b=MOM_B, eps_b=EPS_B):
    """x NCHW (any float dtype, widened exactly), p the parameters by name, running the four old buffers by name or None.
    -> dict of (ref, mag): r (R x C), the four STATS and, with running, the four RUNNING."""
    k = _common(x, p)
    x2, u2, U2, V2, ax, au, av, w1, b1 = (k[n] for n in ("x2", "u2", "U2", "V2", "ax", "au", "av", "w1", "b1"))
    ga, ba, gb, bb = (_d(p[n]) for n in ("gamma_a", "beta_a", "gamma_b", "beta_b"))
    R = x2.shape[0]
    mx, mu = x2.mean(0), u2.mean(0)
    vx, vu = ((x2 - mx) ** 2).mean(0), ((u2 - mu) ** 2).mean(0)
    ia, ib = 1.0 / torch.sqrt(vu + _f32(eps_a)), 1.0 / torch.sqrt(w1 * w1 * vx + _f32(eps_b))
    ka, kb = 1 + au * ia, 1 + av * ib
    uh, vh = (u2 - mu) * ia, w1 * (x2 - mx) * ib
    out = {"mean_x": (mx, ax), "var_x": (vx, vx + ax * torch.sqrt(vx)), "mean_u": (mu, au), "invstd_u": (ia, ia * ka)}
    out["r"] = (ga * uh + ba + gb * vh + bb + x2,
                ga.abs() * (ia * (U2 + au) + uh.abs() * ka) + ba.abs() + gb.abs() * (ib * (V2 + av) + vh.abs() * kb) + bb.abs() + x2.abs())
    if running is not None:
        ma, mb = _f32(mom_a), _f32(mom_b)
        old = [_d(running[n]) for n in RUNNING]
        unb_u, unb_v = vu * R / (R - 1), w1 * w1 * vx * R / (R - 1)
        out["lk_running_mean"] = ((1 - ma) * old[0] + ma * mu, (1 - ma) * old[0].abs() + ma * au)
        out["lk_running_var"] = ((1 - ma) * old[1] + ma * unb_u, (1 - ma) * old[1] + ma * unb_u * ka)
        out["sk_running_mean"] = ((1 - mb) * old[2] + mb * (w1 * mx + b1), (1 - mb) * old[2].abs() + mb * av)
        out["sk_running_var"] = ((1 - mb) * old[3] + mb * unb_v, (1 - mb) * old[3] + mb * unb_v * kb)
    return out


def backward_ref(x, g, p, stats, eps_b=EPS_B):
    """-> dict of (ref, mag): gx (R x C), gw3 (C,1,3,3), gw1 (C) and the other GRADS (C), from the saved float32 stats (4, C) taken as constants."""
    k = _common(x, p)
    x4, x2, u2, U2, V2, ax, au, av, w3, w1 = (k[n] for n in ("x4", "x2", "u2", "U2", "V2", "ax", "au", "av", "w3", "w1"))
    ga, gb = _d(p["gamma_a"]), _d(p["gamma_b"])
    mx, vx, mu, ia = _d(stats)
    g2 = bn64.rows(g)
    R, shape = x2.shape[0], tuple(x4.shape)
    e = _f32(eps_b)
    ib = 1.0 / torch.sqrt(w1 * w1 * vx + e)
    kb = 1 + av * ib
    uh, vh = (u2 - mu) * ia, w1 * (x2 - mx) * ib
    mhu, mhv = (U2 + au) * ia + uh.abs(), ((V2 + av) * ib + vh.abs()) * kb
    ag = g2.abs()
    S0, Su, Sx, Sv = g2.sum(0), (g2 * uh).sum(0), (g2 * (x2 - mx)).sum(0), (g2 * vh).sum(0)
    A0, Au, Av = ag.sum(0), (ag * mhu).sum(0), (ag * mhv).sum(0)
    gu = ga * ia * (g2 - S0 / R - uh * Su / R)
    gv = gb * ib * (g2 - S0 / R - vh * Sv / R)
    mgu = ga.abs() * ia * (ag + A0 / R + uh.abs() * Au / R + mhu * Su.abs() / R)
    mgv = gb.abs() * ib * (ag + A0 / R + vh.abs() * Av / R + mhv * Sv.abs() / R) * kb
    out = {"gbeta_a": (S0, A0), "gbeta_b": (S0, A0), "ggamma_a": (Su, Au), "ggamma_b": (w1 * ib * Sx, Av),
           "gw1": (gb * e * ib ** 3 * Sx, (mgv * x2.abs()).sum(0)), "gb3": (gu.sum(0), mgu.sum(0)), "gb1": (gv.sum(0), mgv.sum(0))}
    gu4, mgu4 = bn64.unrows(gu, shape), bn64.unrows(mgu, shape)
    c = shape[1]
    tr = lambda t, w: F.conv_transpose2d(t.contiguous(), w, padding=1, groups=c)
    out["gx"] = (bn64.rows(tr(gu4, w3)) + w1 * gv + g2, bn64.rows(tr(mgu4, w3.abs())) + w1.abs() * mgv + ag)
    xp, axp = F.pad(x4, (1, 1, 1, 1)), F.pad(x4.abs(), (1, 1, 1, 1))
    h, w = shape[2], shape[3]
    gw, mgw = torch.zeros(c, 1, 3, 3, dtype=torch.float64), torch.zeros(c, 1, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            gw[:, 0, ky, kx] = (gu4 * xp[:, :, ky:ky + h, kx:kx + w]).sum((0, 2, 3))
            mgw[:, 0, ky, kx] = (mgu4 * axp[:, :, ky:ky + h, kx:kx + w]).sum((0, 2, 3))
    out["gw3"] = (gw, mgw)
    return out


def check(got, pair, out_dtype, name):
    """got (NCHW for an R x C reference, (C,1,3,3) for gw3, else C values) against (ref, mag) at grad64's own K; returns the worst ratio."""
    ref, mag = pair
    if ref.dim() == 4:
        return grad64.assert_grad_close(got, ref, mag, out_dtype, name=name, layout="ckk")
    g = bn64.rows(got) if ref.dim() == 2 else got.reshape(-1)
    return grad64.assert_grad_close(g, ref, mag, out_dtype, name=name, layout="rc" if ref.dim() == 2 else "c")
