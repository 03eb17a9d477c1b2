"""Float64 references for the HIP backward kernels, with a per-element error bound.

The reference is autograd in float64 through the ATen restatement (oracle/torch_eager.py) on the very values the HIP path sees (16-bit inputs,
gradients and parameters widened exactly).  A second float64 pass over |x|, |w|, |b| and |gy| gives, for every gradient element, M: the sum of the
absolute values of the products that feed it (every operator in these chains is linear in each operand, with non-negative resize weights).  A
kernel that accumulates in float32 is then held to

    float32 output:  |got - ref| <= K * u32 * M + 2**-150                                    (half the float32 subnormal spacing)
    16-bit output:   |got - ref| <= 1/2 ulp16(max(|ref|, |got|)) + K * u32 * M          (u32 = 2**-24)

which is tight enough to see a truncating store, a one-ulp bias or a wrong border tap whose gradient is far below the plane maximum.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.torch_eager import recconv2d_eager, upadd_dwconv_eager, dwconv_eager

U32 = 2.0 ** -24

# K: about four times the largest err / (u32 * M) measured over tests/test_backward_f64_gpu.py on the MI355X, 6.1 (the float32 input gradient of
# upadd_dwconv_backward at 160 x 64 x 56 x 56; RecConv2d's schedules: 3.9 per-step, 2.5 one-launch 7 x 7, 2.3 tiled 28 x 28, 1.8 tiled 56 x 56,
# 1.5 one-launch 14 x 14, 1.3 generic).  For 16-bit outputs the part of the error beyond half an ulp never exceeded 1.0.
K = 24.0

# significand bits (with the implicit one) and the spacing of the subnormals
_FMT = {torch.bfloat16: (8, 2.0 ** -133), torch.float16: (11, 2.0 ** -24)}
_HALF_SUB32 = 2.0 ** -150


def ulp16(a, dtype):
    """Spacing of `dtype` (bfloat16 / float16) at magnitude |a| (float64 tensor), never below the subnormal spacing."""
    bits, tiny = _FMT[dtype]
    a = a.abs()
    _, e = torch.frexp(a)                            # |a| = m * 2**e, m in [0.5, 1)
    u = torch.clamp(torch.ldexp(torch.ones_like(a), e - bits), min=tiny)
    return torch.where(a > 0, u, torch.full_like(u, tiny))


def grad_bound(got, ref, mag, out_dtype, k=None):
    """Per-element bound (float64, shaped like ref) for an output of dtype out_dtype."""
    k = K if k is None else k
    b = k * U32 * mag
    if out_dtype in _FMT:
        return b + 0.5 * ulp16(torch.maximum(ref.abs(), got.abs()), out_dtype)
    return b + _HALF_SUB32


def _where(idx, shape, layout):
    names = {"nchw": "nchw", "ckk": ("c", "_", "ky", "kx"), "kkc": ("ky", "kx", "c"), "c": ("c",)}.get(layout, None)
    if names is None or len(names) != len(shape):
        return str(idx)
    return "(" + ", ".join(f"{n}={i}" for n, i in zip(names, idx)) + ")"


def assert_grad_close(got, ref64, mag64, out_dtype, k=None, name="grad", layout="nchw"):
    """Check got (any dtype, any device) against ref64 / mag64 (float64) element by element; returns the worst err / (u32 * M), where err is, for a
    16-bit output, what exceeds half an ulp.  layout names got's dimensions in the failure message ("nchw", "ckk" for a (C,1,k,k) weight, "kkc"
    for a packed one, "c")."""
    g = got.detach().to(device=ref64.device, dtype=torch.float64).reshape(ref64.shape)
    ref, mag = ref64.detach(), mag64.detach()
    assert torch.isfinite(g).all(), f"{name}: non-finite values"
    err = (g - ref).abs()
    half = 0.5 * ulp16(torch.maximum(ref.abs(), g.abs()), out_dtype) if out_dtype in _FMT else torch.full_like(err, _HALF_SUB32)
    excess = (err - half).clamp(min=0)
    scale = U32 * mag
    ratio = torch.where(excess > 0, excess / torch.where(scale > 0, scale, torch.ones_like(scale)), torch.zeros_like(excess))
    ratio = torch.where((excess > 0) & (scale == 0), torch.full_like(ratio, float("inf")), ratio)
    bound = grad_bound(g, ref, mag, out_dtype, k)
    bad = err > bound
    if bool(bad.any()):
        viol = torch.where(bad, (err - bound) / torch.where(bound > 0, bound, torch.ones_like(bound)) + (bound == 0).double() * 1e300, torch.zeros_like(err))
        i = int(viol.reshape(-1).argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
        flat = lambda t: float(t.reshape(-1)[i])
        raise AssertionError(
            f"{name} ({out_dtype}): {int(bad.sum())} of {err.numel()} elements outside the bound; worst at {_where(idx, tuple(ref.shape), layout)}: "
            f"got={flat(g):.9g} ref={flat(ref):.9g} |err|={flat(err):.3g} M={flat(mag):.3g} bound={flat(bound):.3g} "
            f"(K={K if k is None else k}; plane max |ref|={float(ref.abs().max()):.3g}; worst err/(u32*M) overall {float(ratio.max()):.3g})")
    return float(ratio.max())


def _run(fn, leaves, gy):
    """float64 autograd of fn(*leaves) . gy twice: as given and on the absolute values -> ([grads], [magnitudes]); None leaves stay None."""
    out = []
    for absolute in (False, True):
        xs = [None if t is None else (t.abs() if absolute else t).detach().to(torch.float64).requires_grad_(True) for t in leaves]
        y = fn(*xs)
        g = gy.abs() if absolute else gy
        live = [t for t in xs if t is not None]
        grads = iter(torch.autograd.grad(y, live, g.detach().to(torch.float64), allow_unused=True))
        res = []
        for t in xs:
            if t is None:
                res.append(None)
                continue
            d = next(grads)
            res.append(torch.zeros_like(t) if d is None else d)
        out.append(res)
    return out[0], out[1]


def recconv2d_grads64(x, gy, w_down, w_convs, b_down=None, b_convs=None, mode="bilinear"):
    """-> (ref, mag): dicts gx, gw [down, convs[0..level]] (C,1,k,k), gb [same order] | None."""
    level = len(w_convs) - 1
    has_b = b_down is not None
    leaves = [x, w_down, *w_convs] + ([b_down, *b_convs] if has_b else [])

    def fn(x_, wd, *rest):
        wc = list(rest[:level + 1])
        if has_b:
            return recconv2d_eager(x_, wd, wc, rest[level + 1], list(rest[level + 2:]), mode)
        return recconv2d_eager(x_, wd, wc, None, None, mode)
    return tuple({"gx": r[0], "gw": r[1:level + 3], "gb": r[level + 3:] if has_b else None} for r in _run(fn, leaves, gy))


def dwconv_grads64(x, gy, w, b=None, stride=1):
    """-> (ref, mag): (gx, gw (C,1,k,k), gb | None)."""
    return _run(lambda x_, w_, b_: dwconv_eager(x_, w_, b_, stride), [x, w, b], gy)


def dwconv_mult2_grads64(x, gy, w, b=None, stride=2):
    """nn.Conv2d(C, 2C, k, stride, k//2, groups=C): -> (ref, mag): (gx, gw (2C,1,k,k), gb | None)."""
    k = w.shape[-1]
    return _run(lambda x_, w_, b_: F.conv2d(x_, w_, b_, stride=stride, padding=k // 2, groups=x_.shape[1]), [x, w, b], gy)


def upadd_dwconv_grads64(x, coarse, gy, w, b=None, mode="nearest"):
    """-> (ref, mag): (gx, gcoarse, gw (C,1,k,k), gb | None)."""
    return _run(lambda x_, c_, w_, b_: upadd_dwconv_eager(x_, c_, w_, b_, mode), [x, coarse, w, b], gy)


def to_kkc(w):
    """(C,1,k,k) -> the kernels' packed (k,k,C) layout, flattened."""
    return w.reshape(w.shape[0], w.shape[-2], w.shape[-1]).permute(1, 2, 0).reshape(-1)
