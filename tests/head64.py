"""Float64 reference for the classifier head (ops.pool_head, ops.global_pool), with the per-element magnitude tests/fwd64.py's bound wants.

From the operands as the kernel sees them -- x rounded to its I/O type, the weight as the pack holds it (float32, or x's type), the bias in float32,
all widened exactly --

    ref[n][k] = b[k] + sum_c w[k][c] * mean_p x[n][p][c]            M[n][k] = |b[k]| + sum_c |w[k][c]| * mean_p |x[n][p][c]|

and the check is fwd64.assert_fwd_close with grad64.K, untouched: a kernel whose arithmetic is float32 and which rounds each output once.
"""
import torch.nn.functional as F

from tests.fwd64 import _pair


def pool_head_fwd64(x, w, b=None):
    """x (N, C, H, W), w (K, C), b (K) | None -> (ref, mag), float64 (N, K)."""
    return _pair(lambda x_, w_, b_: F.linear(x_.mean((2, 3)), w_, b_), [x, w, b])


def global_pool_fwd64(x):
    """x (N, C, H, W) -> (ref, mag), float64 (N, C): the mean and the mean of the absolute values."""
    return _pair(lambda x_: x_.mean((2, 3)), [x])
