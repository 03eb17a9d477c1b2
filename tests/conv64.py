"""Float64 reference and per-element bounds for a depthwise ConvNorm on batch statistics as one operator (rcx_dwconv_bn_train_*; lsnet/model/recattn.py:54-67,
:89-112).  tests/test_conv_norm_cpu.py holds the operator chain on ATen in float32 on the CPU to them, tests/test_conv_norm_gpu.py the HIP kernels.

The reference evaluates the operator's formulas (include/recnext_amd.h) in float64 on the very values the kernel sees: 16-bit inputs and cotangents
widened exactly, eps and momentum as the float32 they are passed as, the nearest resize by the float32 index arithmetic of ATen and
rcx_upadd_dwconv_fwd.  The backward's reference takes the saved float32 statistics (mean u, ia) as given constants, as tests/bn64.py's does.  Every output
comes as (ref, mag) and is checked with tests/grad64.py's assert_grad_close at its K = 24 units of u32 = 2^-24 (never raised: an excess is a kernel bug).
mag follows tests/rep64.py without its sk terms: every sum and product over absolute values, and every quantity that passes through the normalisation
carries bn64's condition factor.  With |z| = |x| + resize |a|, U = sum |w| |z| + |b| the magnitude of u, au = mean U, uhat = (u - mean u) ia,
ka = 1 + au ia, mu = (U + au) ia + |uhat|:

    u        U                  mean u   au                ia   ia ka
    running mean / var          (1 - m) |old| + m au                 (1 - m) old + m var_u R / (R - 1) ka
    y        |gamma| [ia (U + au) + |uhat| ka] + |beta|
    gbeta    sum |g|            ggamma   sum |g| mu
    |gu| = |gamma| ia (|g| + sum |g| / R + |uhat| sum(|g| mu) / R + mu |Su| / R)         Su = sum g uhat
    gw[d]    sum_p |gu|(p) |z|(p s + d - k/2)          gb   sum |gu|  (ref: the float64 sum gu; the operator writes exact zeros)
    gx       sum_d |w[d]| |gu|(p), p s + d - k/2 = q          ga   the resize adjoint of gx's magnitude

Half an ulp of the output type comes on top for a 16-bit output (y, gx)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import bn64, grad64

EXTRA_SHAPES = [(1, 16, 2, 3), (2, 16, 1, 6), (2, 16, 6, 1), (2, 384, 7, 7)]
SHAPES = bn64.SHAPES + EXTRA_SHAPES
# (k, stride, up-add): the slice mixers' pe, a 5x5 at stride 1, down[0], and conv on x + resize(a)
FORMS = [(3, 1, False), (5, 1, False), (5, 2, False), (5, 1, True)]
MOM, EPS = 0.2, 1e-3
GRADS = ("gw", "gb", "ggamma", "gbeta")

_CASES = {}


def out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def coarse_hw(h, w):
    """The size of down[0]'s output: what RecAttn2d hands to the up-add conv."""
    return (h + 1) // 2, (w + 1) // 2


def case(shape, dtype, dist, form):
    """bn64.case's x and, from a seeded generator: g = dL/dy (values of dtype, at the output size), a (float32, at coarse_hw; the up-add form only) and the
    float32 parameters and running buffers.  One weight row is all zeros (that channel's u is its bias: var u = 0), one channel's gamma is 0 and one is
    negative (C = 1: the zero row and the negative gamma meet on the one channel)."""
    key = (shape, dtype, dist, form)
    if key not in _CASES:
        k, stride, up = form
        n, c, h, w = shape
        ho, wo = out_hw(h, w, stride)
        gen = torch.Generator().manual_seed(3000 + sum(shape) * 11 + bn64.DISTS.index(dist) * 5 + FORMS.index(form)
                                            + {torch.float32: 0, torch.bfloat16: 100, torch.float16: 200}[dtype])
        rn = lambda *s: torch.randn(*s, generator=gen)
        d = dict(x=bn64.case(shape, dtype, dist)["x"], g=rn(n, c, ho, wo).to(dtype).float(), w=rn(c, 1, k, k) * (0.9 / k), b=rn(c) * 0.2,
                 gamma=rn(c) * 0.5 + 1.0, beta=rn(c) * 0.3, running_mean=rn(c) * 0.2, running_var=torch.rand(c, generator=gen) + 0.5,
                 a=rn(n, c, *coarse_hw(h, w)) * 0.7 if up else None)
        d["w"][0] = 0.0
        d["gamma"][1 % c] = 0.0
        d["gamma"][2 % c] = -0.75
        _CASES[key] = d
    return _CASES[key]


def _f32(v):
    return float(np.float32(v))


def _d(t):
    return t.detach().double().cpu()


def nearest_index(n_out, n_in):
    """Source index of every destination index of a nearest resize: min(int(float32(d) * (float32(n_in) / float32(n_out))), n_in - 1), ATen's and the
    kernels' arithmetic."""
    scale = np.float32(n_in) / np.float32(n_out)
    idx = (np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, n_in - 1))


def resize(a4, h, w):
    iy, ix = nearest_index(h, a4.shape[2]), nearest_index(w, a4.shape[3])
    return a4[:, :, iy][:, :, :, ix]


def resize_adjoint(g4, hc, wc):
    """The adjoint of resize: every fine pixel's value added to its source pixel."""
    n, c, h, w = g4.shape
    iy, ix = nearest_index(h, hc), nearest_index(w, wc)
    t = torch.zeros(n, c, hc, w, dtype=g4.dtype).index_add_(2, iy, g4)
    return torch.zeros(n, c, hc, wc, dtype=g4.dtype).index_add_(3, ix, t)


def _common(d, form, bias):
    """float64 pieces both references share: z and its magnitude (padded NCHW), u and U (R x C), au."""
    k, stride, up = form
    x4 = _d(d["x"])
    n, c, h, w = x4.shape
    z4, Z4 = x4, x4.abs()
    if up:
        a4 = _d(d["a"])
        z4, Z4 = x4 + resize(a4, h, w), Z4 + resize(a4.abs(), h, w)
    w4 = _d(d["w"])
    b = _d(d["b"]) if bias else None
    conv = lambda t, wt, bt: F.conv2d(t, wt, bt, stride=stride, padding=k // 2, groups=c)
    u4, U4 = conv(z4, w4, b), conv(Z4, w4.abs(), None if b is None else b.abs())
    u2, U2 = bn64.rows(u4), bn64.rows(U4)
    return dict(z4=z4, Z4=Z4, w4=w4, u4=u4, u2=u2, U2=U2, au=U2.mean(0), shape=(n, c, h, w), oshape=tuple(u4.shape))


def forward_ref(d, form, bias=True, running=True, mom=MOM, eps=EPS):
    """d: a case (x NCHW of any float dtype, widened exactly).  -> dict of (ref, mag): y and u (R x C), mean_u, invstd_u and, with running, running_mean
    and running_var."""
    k = _common(d, form, bias)
    u2, U2, au = k["u2"], k["U2"], k["au"]
    ga, be = _d(d["gamma"]), _d(d["beta"])
    R = u2.shape[0]
    mu = u2.mean(0)
    vu = ((u2 - mu) ** 2).mean(0)
    ia = 1.0 / torch.sqrt(vu + _f32(eps))
    ka = 1 + au * ia
    uh = (u2 - mu) * ia
    out = {"u": (u2, U2), "mean_u": (mu, au), "invstd_u": (ia, ia * ka),
           "y": (ga * uh + be, ga.abs() * (ia * (U2 + au) + uh.abs() * ka) + be.abs())}
    if running:
        m = _f32(mom)
        rm, rv = _d(d["running_mean"]), _d(d["running_var"])
        unb = vu * R / (R - 1)
        out["running_mean"] = ((1 - m) * rm + m * mu, (1 - m) * rm.abs() + m * au)
        out["running_var"] = ((1 - m) * rv + m * unb, (1 - m) * rv + m * unb * ka)
    return out


def backward_ref(d, form, stats, bias=True):
    """-> dict of (ref, mag): gx (R_in x C), ga (R_coarse x C; the up-add form), gw (C,1,k,k) and the other GRADS (C), from the saved float32 stats (2, C)
    taken as constants."""
    ks, stride, up = form
    k = _common(d, form, bias)
    u2, U2, au, w4 = k["u2"], k["U2"], k["au"], k["w4"]
    n, c, h, w = k["shape"]
    oshape = k["oshape"]
    ho, wo = oshape[2], oshape[3]
    ga = _d(d["gamma"])
    mu, ia = _d(stats)
    g2 = bn64.rows(d["g"])
    R = u2.shape[0]
    uh = (u2 - mu) * ia
    mhu = (U2 + au) * ia + uh.abs()
    ag = g2.abs()
    S0, Su = g2.sum(0), (g2 * uh).sum(0)
    A0, Au = ag.sum(0), (ag * mhu).sum(0)
    gu = ga * ia * (g2 - S0 / R - uh * Su / R)
    mgu = ga.abs() * ia * (ag + A0 / R + uh.abs() * Au / R + mhu * Su.abs() / R)
    out = {"gbeta": (S0, A0), "ggamma": (Su, Au), "gb": (gu.sum(0), mgu.sum(0))}
    gu4, mgu4 = bn64.unrows(gu, oshape).contiguous(), bn64.unrows(mgu, oshape).contiguous()
    p = ks // 2
    opad = (h - ((ho - 1) * stride - 2 * p + ks), w - ((wo - 1) * stride - 2 * p + ks))
    tr = lambda t, wt: F.conv_transpose2d(t, wt, stride=stride, padding=p, output_padding=opad, groups=c)
    gz4, mgz4 = tr(gu4, w4), tr(mgu4, w4.abs())
    out["gx"] = (bn64.rows(gz4), bn64.rows(mgz4))
    if up:
        hc, wc = d["a"].shape[2], d["a"].shape[3]
        out["ga"] = (bn64.rows(resize_adjoint(gz4, hc, wc)), bn64.rows(resize_adjoint(mgz4, hc, wc)))
    zp, Zp = F.pad(k["z4"], (p, p, p, p)), F.pad(k["Z4"], (p, p, p, p))
    gw, mgw = torch.zeros(c, 1, ks, ks, dtype=torch.float64), torch.zeros(c, 1, ks, ks, dtype=torch.float64)
    for ky in range(ks):
        for kx in range(ks):
            sl = (slice(None), slice(None), slice(ky, ky + stride * (ho - 1) + 1, stride), slice(kx, kx + stride * (wo - 1) + 1, stride))
            gw[:, 0, ky, kx] = (gu4 * zp[sl]).sum((0, 2, 3))
            mgw[:, 0, ky, kx] = (mgu4 * Zp[sl]).sum((0, 2, 3))
    out["gw"] = (gw, mgw)
    return out


def check(got, pair, out_dtype, name):
    """got (NCHW for an R x C reference, (C,1,k,k) for gw, else C values) against (ref, mag) at grad64's own K; returns the worst ratio."""
    ref, mag = pair
    if ref.dim() == 4:
        return grad64.assert_grad_close(got, ref, mag, out_dtype, name=name, layout="ckk")
    g = bn64.rows(got) if ref.dim() == 2 else got.reshape(-1)
    return grad64.assert_grad_close(g, ref, mag, out_dtype, name=name, layout="rc" if ref.dim() == 2 else "c")
