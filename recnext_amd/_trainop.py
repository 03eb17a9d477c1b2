"""What the training-step operators (batchnorm.py, repdw.py, dwbn.py, bnact.py; ``ptr`` also lsdown.py and head.py) share between a tensor and a C
entry: pointers, the cached support query, the workspace, the routing-table lookup, the argument checks and the gradient plumbing of the Functions.

Why those operators' functions are written in modules of their own and not in ops.py, which exports them: tests/test_guard_cpu.py asks a row in the
case table of tests/test_guard_bands_gpu.py of every launching function whose source is in ops.py, and these entries' guard-band cases are in each
operator's own GPU test, which passes the operator's module to tests/guard.py as one of ``modules=``.  Nothing is allocated here: the workspace and the
parameter-gradient block are ops._empty_flat's, the dense outputs ops._empty_nhwc's (ops.py is one of guard.LIBRARY_MODULES), the (C) vectors the
operator modules' own ``torch.empty``, so the guard sees every allocation where it always looked."""
import functools
import math

import torch

from . import _lib, ops


def ptr(t):
    return t.data_ptr() if t is not None else None


def esize(dtype):
    """The element size a routing table keys on: 4 for float32, 2 for bfloat16 and float16."""
    return 4 if dtype == torch.float32 else 2


def rows_routed(table, key, rows):
    """Whether a routing table (key -> (lo, hi), both inclusive) keeps `rows` for `key`; a key that is not in it keeps nothing."""
    lo, hi = table.get(key, (1, 0))
    return lo <= rows <= hi


@functools.lru_cache(maxsize=4096)
def supported(query, *args):
    """The library's ``rcx_*_supported`` query `query` of integer arguments (extents, dtype codes): a rule on its arguments alone, so asked of the
    library once a shape."""
    return getattr(_lib.load(), query)(*map(int, args)) > 0


def workspace(query, device, *args):
    """-> (uint8 tensor, nbytes) of the size the library's ``rcx_*_workspace_bytes`` query `query` gives for args."""
    nbytes = getattr(_lib.load(), query)(*args)
    return ops._empty_flat(nbytes, torch.uint8, device), nbytes


def gpu_tensor_ok(x):
    """A 4-D GPU tensor of a dtype the kernels take: what every module-level gate asks of its input first."""
    return torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in ops._DT


def dense_nhwc(t):
    n, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    return all(sz == 1 or st == wt for sz, st, wt in zip(t.shape, t.stride(), want))


def check_x(fn, x, name="x"):
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"{fn}: {name} must be a 4-D (N, C, H, W) tensor")
    if x.dtype not in ops._DT:
        raise ValueError(f"{fn}: {name} must be float32, bfloat16 or float16, got {x.dtype}")
    ops._require_gpu(x, name)
    if x.numel() == 0:
        raise ValueError(f"{fn}: {name} is empty, shape {tuple(x.shape)}")
    if not dense_nhwc(x):
        raise ValueError(f"{fn}: {name} must be dense channels_last (N x H x W x C storage), got shape {tuple(x.shape)} strides {x.stride()}")


def check_vec(fn, t, c, device, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (c,) or t.device != device or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be a contiguous float32 ({c},) tensor on {device}")


def check_like(fn, t, name, shape, dtypes, device):
    """A gradient or a residual: a dense channels_last tensor (check_x) of this shape, one of these dtypes, on this device."""
    check_x(fn, t, name)
    if tuple(t.shape) != tuple(shape) or t.dtype not in dtypes or t.device != device:
        raise ValueError(f"{fn}: {name} is {tuple(t.shape)} {t.dtype} on {t.device}, wanted {tuple(shape)} {' or '.join(map(str, dtypes))} on {device}")


def check_running(fn, bufs, c, device, names):
    """The running buffers `names` of a call, None standing for as many None: float32 (C) each, all of them or none.  -> their pointers."""
    bufs = (None,) * len(names) if bufs is None else tuple(bufs)
    if len(bufs) != len(names) or len({t is None for t in bufs}) != 1:
        raise ValueError(f"{fn}: {' and '.join(names)} come together or not at all")
    for name, t in zip(names, bufs):
        if t is not None:
            check_vec(fn, t, c, device, name)
    return [ptr(t) for t in bufs]


def check_dw_weight(fn, w, c, device, name, k=None):
    """A depthwise conv's weight: contiguous float32 (C, 1, k, k), k its own where None is given.  -> k"""
    if not torch.is_tensor(w) or w.dtype != torch.float32 or w.dim() != 4 or tuple(w.shape) != (c, 1, k or w.shape[-1], k or w.shape[-1]) \
            or w.device != device or not w.is_contiguous():
        raise ValueError(f"{fn}: {name} must be a contiguous float32 ({c}, 1, {k or 'k'}, {k or 'k'}) tensor on {device}")
    return w.shape[-1]


def check_rows(rows, size):
    """Batch statistics of one value a channel are refused, as torch refuses them, in torch's words; `size` is what the message shows."""
    if rows == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {size}")


def grad_in(g, dtype, name="g"):
    """An incoming gradient as the entries want it: of `dtype` (cast only if it is not) and dense channels_last."""
    if g.dtype != dtype:
        g = g.to(dtype)
    return g if dense_nhwc(g) else ops._nhwc(g, name)


def carve_f32(shapes, device):
    """One float32 buffer holding tensors of `shapes` back to back (one allocation, one finalize kernel) -> (its views, their pointers)."""
    sizes = [math.prod(s) for s in shapes]
    buf = ops._empty_flat(sum(sizes), torch.float32, device)
    starts = [sum(sizes[:i]) for i in range(len(sizes))]
    return tuple(buf[o:o + k].view(s) for o, k, s in zip(starts, sizes, shapes)), [buf.data_ptr() + 4 * o for o in starts]


def grads_out(grads, dtypes, need):
    """The float32 parameter gradients `grads` (or None) for a Function's return: each in its parameter's dtype, None where it is not needed or
    the parameter does not exist (dtype None)."""
    if grads is None:
        return [None] * len(dtypes)
    return [t.to(dt) if nd and dt is not None else None for t, dt, nd in zip(grads, dtypes, need)]
