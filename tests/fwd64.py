"""Float64 references for the linear HIP forward kernels, with the per-element error bound of tests/grad64.py.

The reference is the ATen restatement (oracle/torch_eager.py; F.conv2d for the channel-multiplier-2 and the grouped conv) in float64 on the very
values the kernel sees: activations rounded to their I/O type and widened exactly, weights and biases as the float32 packs hold them.  A second
float64 pass over |x|, |w|, |b| and |coarse| gives, for every output element, M: the sum of the absolute values of the products that feed it (every
operator here is linear in each operand and the resize weights are non-negative, so the absolute values pass through every level of a ladder).  A
kernel whose arithmetic is float32 and which rounds each output once at its store is then held to grad64's bound,

    float32 output:  |got - ref| <= K * u32 * M + 2**-150
    16-bit output:   |got - ref| <= 1/2 ulp16(max(|ref|, |got|)) + K * u32 * M          (u32 = 2**-24, K = grad64.K)

which sees a truncating store, a float16 output that went through bfloat16, a coarse plane held in 16 bits, a dropped border tap on a pixel far
below the plane maximum and a bias added twice; tests/test_fwd_bound_cpu.py plants each of them.
"""
import torch
import torch.nn.functional as F

from oracle.torch_eager import dwconv_eager, recconv2d_eager, upadd_dwconv_eager
from tests.grad64 import K, U32, assert_grad_close          # noqa: F401  (K and U32 are re-exported: the constant is grad64's, not tuned here)

# the forward-facing name of the check: the same function, the same bound
assert_fwd_close = assert_grad_close


def _pair(fn, operands):
    """fn on the operands widened to float64, then on their absolute values -> (ref, mag); None operands stay None."""
    out = []
    for absolute in (False, True):
        def widen(t):
            if t is None:
                return None
            if isinstance(t, (list, tuple)):
                return [widen(u) for u in t]
            t = t.detach().to(device="cpu", dtype=torch.float64)
            return t.abs() if absolute else t
        with torch.no_grad():
            out.append(fn(*[widen(t) for t in operands]))
    return out[0], out[1]


def recconv2d_fwd64(x, w_down, w_convs, b_down=None, b_convs=None, mode="bilinear"):
    """RecConv2d.forward: x (N,C,H,W), weights (C,1,k,k), biases (C) | None -> (ref, mag), float64 (N,C,H,W)."""
    return _pair(lambda x_, wd, wc, bd, bc: recconv2d_eager(x_, wd, wc, bd, bc, mode), [x, w_down, list(w_convs), b_down, None if b_convs is None else list(b_convs)])


def dwconv_fwd64(x, w, b=None, stride=1):
    """Depthwise conv, pad k // 2: w (C,1,k,k) -> (ref, mag)."""
    return _pair(lambda x_, w_, b_: dwconv_eager(x_, w_, b_, stride), [x, w, b])


def dwconv_mult2_fwd64(x, w, b=None, stride=2):
    """nn.Conv2d(C, 2C, k, stride, k // 2, groups=C): w (2C,1,k,k) -> (ref, mag)."""
    k = w.shape[-1]
    return _pair(lambda x_, w_, b_: F.conv2d(x_, w_, b_, stride=stride, padding=k // 2, groups=x_.shape[1]), [x, w, b])


def upadd_dwconv_fwd64(x, coarse, w, b=None, mode="nearest"):
    """conv_k(x + resize(coarse)), or conv_k(x) for coarse None: -> (ref, mag)."""
    if coarse is None:
        return dwconv_fwd64(x, w, b, 1)
    return _pair(lambda x_, c_, w_, b_: upadd_dwconv_eager(x_, c_, w_, b_, mode), [x, coarse, w, b])


def grouped_conv2d_fwd64(x, w, b=None, groups=1, stride=2):
    """nn.Conv2d(Cin, Cout, k, stride, k // 2, groups=groups): w (Cout, Cin / groups, k, k) -> (ref, mag)."""
    k = w.shape[-1]
    return _pair(lambda x_, w_, b_: F.conv2d(x_, w_, b_, stride=stride, padding=k // 2, groups=groups), [x, w, b])


def legacy_bar_holds(got, ref, out_dtype):
    """The bars this bound replaces (tests/test_recconv_gpu.py, tests/test_ls_down_gpu.py): float32 max|err| < 1e-4 over the tensor, 16-bit
    |err| <= 1e-2 + 1e-2 |ref| per element.  Kept only so that tests/test_fwd_bound_cpu.py can show what they let through."""
    err = (got.detach().to(device="cpu", dtype=torch.float64).reshape(ref.shape) - ref).abs()
    if out_dtype == torch.float32:
        return bool(err.max() < 1e-4)
    return bool((err <= 1e-2 + 1e-2 * ref.abs()).all())
