"""Float64 references and per-element bounds for the BatchNorm epilogues of recnext_amd/bnact.py, built on tests/bn64.py and tests/grad64.py
(tests/test_bnact_cpu.py holds ATen's float32 chain to them on the CPU, tests/test_bnact_gpu.py the HIP kernels on the GPU).  K = tests/grad64.py's 24,
u32 = 2^-24, half an ulp on top for a 16-bit output (assert_grad_close); K is not to be raised.

bn_gelu forward    save_mean, save_invstd, the running buffers: bn64.forward_ref's bounds.  With (y64, mag_y) = forward_ref(...)["y"]:
                   z = gelu(y64), magnitude 1.13 mag_y + |y64|: sup |gelu'| = 1.129 carries y's error into z, and |y64| the erf's absolute error
                   (z = y (1 + erf(y / sqrt 2)) / 2: an error e of erf moves z by |y| e / 2, so 24 u32 |y64| leaves erf about 2.8e-6).
bn_gelu backward   the kernel's saved float32 mean and invstd taken as constants (as bn64.backward_ref): y64 = xhat gamma + beta,
                   my = |gamma| r (|u| + |mean|) + |beta|, d = gz gelu'(y64), dm = |d| + |gz| (1 + 0.8 my): sup |gelu''| = 0.798 carries y's error
                   into gelu', the 1 the evaluation of gelu' itself.  Then bn64.backward_ref's formulas with d for gy in the references and dm for
                   |gy| in the magnitudes.
bn_add             forward r + s y64, magnitude |s| mag_y + |r|; backward bn64.backward_ref as it is with gy := s (.) g in float64; gr is g itself."""
import math

import torch

from tests import bn64

KEEP = 0.8                                               # the DropPath keep probability of the scaled cases: 1 / KEEP = 1.25 exactly in every dtype


def gelu64(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def dgelu64(y):
    return 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0))) + y * torch.exp(-0.5 * y * y) / math.sqrt(2.0 * math.pi)


_EXTRA = {}


def extra(shape, dtype, dist):
    """The residual r (float32 NCHW values representable in dtype) and the DropPath scale (float32 (N): an exact 0 first, 1 / KEEP after) of one case,
    made once beside bn64.case's tensors and left unchanged."""
    key = (shape, dtype, dist)
    if key not in _EXTRA:
        gen = torch.Generator().manual_seed(sum(shape) * 7 + 3 * bn64.DISTS.index(dist) + {torch.float32: 1, torch.bfloat16: 101, torch.float16: 201}[dtype])
        r = (torch.randn(*shape, generator=gen) * 1.5 + 0.25).to(dtype).float()
        scale = torch.full((shape[0],), 1.0 / KEEP)
        scale[0] = 0.0
        _EXTRA[key] = dict(r=r, scale=scale)
    return _EXTRA[key]


def per_row(scale, shape):
    """float32 (N) -> float64 R x 1: the scale of every row."""
    n, c, h, w = shape
    return scale.detach().double().cpu().view(n, 1, 1).expand(n, h * w, 1).reshape(-1, 1)


def gelu_forward_ref(x, weight, bias, eps, running_mean=None, running_var=None, momentum=bn64.MOMENTUM):
    """-> bn64.forward_ref's dict with "z" in place of "y"."""
    out = bn64.forward_ref(x, weight, bias, eps, running_mean=running_mean, running_var=running_var, momentum=momentum)
    y, mag = out.pop("y")
    out["z"] = (gelu64(y), 1.13 * mag + y.abs())
    return out


def gelu_backward_ref(u, gz, weight, bias, mean, invstd):
    """-> dict of (ref, mag): gx (R x C), gweight, gbias (C), from the kernel's saved float32 mean and invstd taken as constants."""
    x2, gz2 = bn64.rows(u), bn64.rows(gz)
    g, b = weight.detach().double().cpu(), bias.detach().double().cpu()
    mu, r = mean.detach().double().cpu(), invstd.detach().double().cpu()
    R = x2.shape[0]
    a = x2.abs().mean(0)
    xh = (x2 - mu) * r
    mh = (x2.abs() + a) * r + xh.abs()
    y = xh * g + b
    my = g.abs() * r * (x2.abs() + mu.abs()) + b.abs()
    d = gz2 * dgelu64(y)
    dm = d.abs() + gz2.abs() * (1.0 + 0.8 * my)
    sg, sgx = d.sum(0), (d * xh).sum(0)
    return {"gbias": (sg, dm.sum(0)), "gweight": (sgx, (dm * mh).sum(0)),
            "gx": (g * r * (d - sg / R - xh * sgx / R), g.abs() * r * (dm + dm.sum(0) / R + xh.abs() * (dm * mh).sum(0) / R + mh * sgx.abs() / R))}


def add_forward_ref(x, res, scale, weight, bias, eps, running_mean=None, running_var=None, momentum=bn64.MOMENTUM):
    """scale: float32 (N) or None.  -> bn64.forward_ref's dict with "out" in place of "y"."""
    out = bn64.forward_ref(x, weight, bias, eps, running_mean=running_mean, running_var=running_var, momentum=momentum)
    y, mag = out.pop("y")
    r2 = bn64.rows(res)
    s = per_row(scale, x.shape) if scale is not None else torch.ones(r2.shape[0], 1, dtype=torch.float64)
    out["out"] = (r2 + s * y, s.abs() * mag + r2.abs())
    return out


def add_backward_ref(u, g, scale, weight, mean, invstd):
    """bn64.backward_ref as it is with gy := s (.) g in float64."""
    gy = g.detach().double().cpu()
    if scale is not None:
        gy = gy * scale.detach().double().cpu().view(-1, 1, 1, 1)
    return bn64.backward_ref(u, gy, weight, mean, invstd, True)
