"""Float64 references and per-element bounds for BatchNorm on an R x C operand (tests/test_batchnorm_cpu.py holds torch.native_batch_norm to them on the
CPU, tests/test_batchnorm_gpu.py the HIP kernels on the GPU).

The reference evaluates the textbook formulas in float64 on the very values the kernel sees: 16-bit inputs widened exactly, eps as the float32 it is passed
as.  The backward's reference takes the kernel's own saved float32 mean and invstd as given constants.  With u32 = 2^-24, K = tests/grad64.py's 24,
a = mean |x| of the channel, r = the float64 invstd, xhat = (x - mean) r, m = momentum, rm = the old running value, var = the new (biased) statistic,
mh = (|x| + a) r + |xhat|:

    save_mean              K u32 a
    save_invstd            K u32 r (1 + a r)
    running_mean           K u32 ((1 - m) |rm| + m a)
    running_var            K u32 ((1 - m) rm + m (var R / (R - 1)) (1 + a r))
    y                      K u32 (|gamma| [r (|x| + a) + |xhat| (1 + a r)] + |beta|)
    gbeta                  K u32 sum |gy|
    ggamma                 K u32 sum |gy| mh
    gx (batch statistics)  K u32 |gamma| r (|gy| + sum |gy| / R + |xhat| (sum |gy| mh) / R + mh |ggamma| / R)
    gx (frozen)            K u32 |gamma r gy|

and half an ulp of the output type on top for a 16-bit output (tests/grad64.py's assert_grad_close adds it, and 2^-150 for a float32 one).  A one-pass
E[x^2] - mean^2 misses the invstd bound by 20 - 35 x on the two ill-conditioned float32 distributions; ATen's float32 BatchNorm stays at or below 6.9 of
the 24 units.  K is not to be raised: an excess is a kernel bug."""
import numpy as np
import torch

from tests import grad64

SHAPES = [(2, 8, 1, 1), (3, 21, 5, 9), (5, 1, 3, 3), (2, 24, 7, 7), (5, 16, 13, 11), (8, 40, 14, 14), (2, 16, 56, 56), (64, 8, 14, 14), (4, 768, 4, 4)]
UNALIGNED = (2, 16, 5, 7)             # run on a dense tensor whose pointer is one element past a 16-byte boundary
DISTS = ("normal", "offsets", "near2", "const0")
MOMENTUM, EPS = 0.1, 1e-5


def dists_of(dtype):
    return DISTS if dtype == torch.float32 else tuple(d for d in DISTS if d != "near2")


def make_x(shape, dtype, dist, gen):
    """float32 NCHW values representable in dtype."""
    n, c, h, w = shape
    x = torch.randn(n, c, h, w, generator=gen)
    if dist == "offsets":                                  # per-channel offsets across +-1000 sigma (float32), +-8 sigma (16-bit)
        span = 1000.0 if dtype == torch.float32 else 8.0
        x = x + torch.linspace(-span, span, c).view(1, c, 1, 1)
    elif dist == "near2":
        x = 2.0 + 1e-3 * x
    elif dist == "const0":                                 # one constant channel and one all-zero channel (C = 1: the constant one)
        x[:, 0] = 0.75
        if c > 1:
            x[:, c - 1] = 0.0
    return x.to(dtype).float()


_CASES = {}


def case(shape, dtype, dist):
    """The inputs of one case, made once on the CPU: float32 tensors holding values of dtype (x, gy: NCHW) and float32 parameters and running buffers."""
    key = (shape, dtype, dist)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(sum(shape) * 13 + DISTS.index(dist) + {torch.float32: 0, torch.bfloat16: 100, torch.float16: 200}[dtype])
        c = shape[1]
        _CASES[key] = dict(x=make_x(shape, dtype, dist, gen), gy=torch.randn(*shape, generator=gen).to(dtype).float(),
                           weight=torch.randn(c, generator=gen) * 0.5 + 1.0, bias=torch.randn(c, generator=gen) * 0.3,
                           running_mean=torch.randn(c, generator=gen) * 0.2, running_var=torch.rand(c, generator=gen) + 0.5)
    return _CASES[key]


def rows(t):
    """NCHW -> float64 R x C."""
    return t.detach().double().cpu().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def unrows(t2, shape):
    n, c, h, w = shape
    return t2.reshape(n, h, w, c).permute(0, 3, 1, 2)


def _eps64(eps):
    return float(np.float32(eps))


def forward_ref(x, weight, bias, eps, mean=None, var=None, running_mean=None, running_var=None, momentum=MOMENTUM):
    """x NCHW (any float dtype, widened exactly).  Batch statistics unless mean and var (the frozen form's float32 statistics) are given.
    -> dict of (ref, mag) pairs in float64, mag the bound divided by K u32: y (R x C), and for batch statistics save_mean, save_invstd and, with running
    buffers, running_mean and running_var."""
    x2, g, b = rows(x), weight.detach().double().cpu(), bias.detach().double().cpu()
    R = x2.shape[0]
    a = x2.abs().mean(0)
    out = {}
    if mean is None:
        mu = x2.mean(0)
        v = ((x2 - mu) ** 2).mean(0)
    else:
        mu, v = mean.detach().double().cpu(), var.detach().double().cpu()
    r = 1.0 / torch.sqrt(v + _eps64(eps))
    xh = (x2 - mu) * r
    out["y"] = (xh * g + b, g.abs() * (r * (x2.abs() + a) + xh.abs() * (1 + a * r)) + b.abs())
    if mean is None:
        out["save_mean"] = (mu, a)
        out["save_invstd"] = (r, r * (1 + a * r))
        if running_mean is not None:
            rm, rv, m = running_mean.detach().double().cpu(), running_var.detach().double().cpu(), float(np.float32(momentum))
            unb = v * R / (R - 1)
            out["running_mean"] = ((1 - m) * rm + m * mu, (1 - m) * rm.abs() + m * a)
            out["running_var"] = ((1 - m) * rv + m * unb, (1 - m) * rv + m * unb * (1 + a * r))
    return out


def backward_ref(x, gy, weight, mean, invstd, batch_stats):
    """-> dict of (ref, mag): gx (R x C), gweight, gbias (C), from the kernel's saved float32 mean and invstd taken as constants."""
    x2, d, g = rows(x), rows(gy), weight.detach().double().cpu()
    mu, r = mean.detach().double().cpu(), invstd.detach().double().cpu()
    R = x2.shape[0]
    a = x2.abs().mean(0)
    xh = (x2 - mu) * r
    mh = (x2.abs() + a) * r + xh.abs()
    sg, sgx = d.sum(0), (d * xh).sum(0)
    out = {"gbias": (sg, d.abs().sum(0)), "gweight": (sgx, (d.abs() * mh).sum(0))}
    if batch_stats:
        out["gx"] = (g * r * (d - sg / R - xh * sgx / R),
                     g.abs() * r * (d.abs() + d.abs().sum(0) / R + xh.abs() * (d.abs() * mh).sum(0) / R + mh * sgx.abs() / R))
    else:
        out["gx"] = (g * r * d, (g * r * d).abs())
    return out


def check(got, pair, out_dtype, name):
    """got (NCHW for an R x C reference, else (C)) against (ref, mag): tests/grad64.py's per-element bound at its own K; returns the worst ratio."""
    ref, mag = pair
    g = rows(got) if got.dim() == 4 else got
    return grad64.assert_grad_close(g, ref, mag, out_dtype, name=name, layout="rc" if ref.dim() == 2 else "c")
