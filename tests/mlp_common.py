"""What the channel mixer's GPU tests (tests/test_mlp*_gpu.py) share: the device, seeded bf16 operands, the float64 formula and the bf16 bar.  A plain module,
imported by name (as tests/guard.py)."""
import math

import torch


def dev():
    return torch.device("cuda:0")


def operands(n, c, hid, h, w, seed):
    """z, x (N x C x H x W, channels_last), w1 (hid x C), b1, w2 (C x hid), b2: bf16 on the device, drawn in this order from one CPU generator."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rb = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(torch.bfloat16)
    z = rb(n, c, h, w).to(dev()).contiguous(memory_format=torch.channels_last)
    x = rb(n, c, h, w).to(dev()).contiguous(memory_format=torch.channels_last)
    w1, b1 = rb(hid, c, sc=(2.0 / c) ** 0.5).to(dev()), rb(hid, sc=0.3).to(dev())
    w2, b2 = rb(c, hid, sc=(1.0 / hid) ** 0.5).to(dev()), rb(c, sc=0.3).to(dev())
    return z, x, w1, b1, w2, b2


def reference(z, x, w1, b1, w2, b2):
    """float64 on the CPU: the operands as the kernel sees them (bf16 values), exact erf GELU, no intermediate rounding."""
    z64, x64 = z.double().cpu(), x.double().cpu()
    n, c, h, w = z64.shape
    zz = z64.permute(0, 2, 3, 1).reshape(-1, c)
    hid = zz @ w1.double().cpu().t() + b1.double().cpu()
    hid = 0.5 * hid * (1.0 + torch.erf(hid / math.sqrt(2.0)))
    out = hid @ w2.double().cpu().t() + b2.double().cpu()
    return x64 + out.reshape(n, h, w, c).permute(0, 3, 1, 2)


def check(y, ref, what):
    """|y - ref| <= 1e-2 + 1e-2 |ref| at every element (north_star's bf16 bar); prints the figures first and returns |y - ref| for the caller's further bounds."""
    err = (y.double().cpu() - ref).abs()
    tol = 1e-2 + 1e-2 * ref.abs()
    print(f"\n{what}: worst err / tol {float((err / tol).max()):.3f}, max |ref| {float(ref.abs().max()):.2f}, mean |err| {float(err.mean()):.2e}")
    assert bool((err <= tol).all())
    return err
