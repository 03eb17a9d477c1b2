"""The classifier head behind the last block as one HIP launch (rcx_pool_head_fwd, recnext_amd/csrc/rcx_head.hip): global average pool + linear,
``head(x.mean((2, 3)))`` of model/recnext.py's forward_head / RecNextClassifier and of lsnet/model/recattn.py:266-293, :307-387, in float32 arithmetic
with one rounding at the store; and the pool alone (rcx_global_pool_fwd) for ``num_classes=0``.  ``FusedHead`` is the model-side helper
``models.use_fused_head`` attaches.

recnext_amd.ops exports the functions (``ops.pool_head`` ...); they are written here because tests/test_guard_cpu.py asks a row in the case table of
tests/test_guard_bands_gpu.py of every launching function whose source is in ops.py, and these entries' guard-band cases are in
tests/test_head_gpu.py, which passes this module to tests/guard.py as one of ``modules=`` (as recnext_amd/dwbn.py does): the outputs are allocated by
this module's own ``torch.empty``.  A CPU tensor raises; there is no fallback."""
import torch

from . import _lib, ops
from ._trainop import esize, ptr, rows_routed

# The routing rule (profiles/r25_head.txt): (C, H W, element size of x) -> the batch sizes N from the smallest to the largest at
# which the launch beat the library chain (mean + F.linear) by more than the chain's own spread in that job, both from Python (device events around
# eager calls) and replayed in a HIP graph (the GPU's side alone); measured at N = 1, 8, 64 and 256, bf16, K = 1000.  No timing at run time.  A shape
# that is not here stays on the chain unless ``use_fused_head(net, all_shapes=True)`` asks for every shape the kernel takes.  Left out: every shape at
# N = 256 (0.44 - 0.73 x in the graph: x is pooled again by every class tile and w read again by every image tile), C = 640 (0.44 - 0.98 x in the graph
# at every N), 16 x 16 planes at N = 32 (0.79 x), and the widths (384, 448) and element sizes (float32) nobody measured.
ROUTED = {(320, 49, 2): (1, 64), (512, 49, 2): (1, 64), (512, 16, 2): (1, 64)}


def pool_head_routed(n, h, w, c, k, dtype):
    """Whether the routing rule keeps the shape on the HIP head: a rule on (N, H W, C, element size) alone."""
    return rows_routed(ROUTED, (int(c), int(h) * int(w), esize(dtype)), int(n))          # this table's bounds are batch sizes


def pool_head_supported(n, h, w, c, k, dtype, wdtype=None, measured_only=False):
    """Whether rcx_pool_head_fwd takes x of (N, H, W, C) and dtype with a (K, C) weight of wdtype (default: dtype): C a multiple of 8 up to 1024, the
    weight float32 or of x's type, fewer than 2^31 elements; with measured_only, also whether the routing rule keeps it (pool_head_routed)."""
    wdtype = dtype if wdtype is None else wdtype
    if dtype not in ops._DT or wdtype not in ops._DT:
        return False
    if _lib.load().rcx_pool_head_supported(int(n), int(h), int(w), int(c), int(k), ops._DT[dtype], ops._DT[wdtype]) <= 0:
        return False
    return not measured_only or pool_head_routed(n, h, w, c, k, dtype)


def _key(tensors):
    return tuple(None if t is None else (t.data_ptr(), t._version, t.dtype, t.device, tuple(t.shape)) for t in tensors)


def _norm_linear_parts(nl):
    """The tensors a NormLinear's eval-mode function depends on: the BatchNorm1d's four and the Linear's two."""
    return [nl.norm.weight, nl.norm.bias, nl.norm.running_mean, nl.norm.running_var, nl.linear.weight, nl.linear.bias]


def _fold_norm_linear(nl, dtype):
    """NormLinear.fuse()'s arithmetic in `dtype`: (W scale, W shift + b) of the eval-mode BatchNorm1d folded into the Linear."""
    n = nl.norm
    one = torch.ones_like(n.running_var, dtype=dtype)
    gamma = n.weight.detach().to(dtype) if n.weight is not None else one
    beta = n.bias.detach().to(dtype) if n.bias is not None else torch.zeros_like(one)
    scale = gamma / torch.sqrt(n.running_var.detach().to(dtype) + n.eps)
    shift = beta - scale * n.running_mean.detach().to(dtype)
    w = nl.linear.weight.detach().to(dtype)
    b = w @ shift
    if nl.linear.bias is not None:
        b = b + nl.linear.bias.detach().to(dtype)
    return w * scale.view(1, -1), b


def fold_classifier(head, dtype=torch.float32):
    """RecNextClassifier.fuse()'s arithmetic, done once in `dtype`: both BatchNorms folded, the two heads averaged -> (weight (K, C), bias (K))."""
    wa, ba = _fold_norm_linear(head.head, dtype)
    wb, bb = _fold_norm_linear(head.head_dist, dtype)
    return (wa + wb) / 2, (ba + bb) / 2


def _is_unfused_classifier(head):
    from .layers import NormLinear
    from .models import RecNextClassifier
    if type(head) is not RecNextClassifier:
        return False
    for nl in (head.head, head.head_dist):
        if type(nl) is not NormLinear or type(nl.norm) is not torch.nn.BatchNorm1d or type(nl.linear) is not torch.nn.Linear:
            return False
        if nl.norm.running_mean is None or nl.norm.running_var is None:
            return False
    return True


def head_tensors(head):
    """The parameters and buffers the head's eval-mode function depends on, for an nn.Linear or an unfused RecNextClassifier; None for anything else."""
    if type(head) is torch.nn.Linear:
        return [head.weight, head.bias]
    if _is_unfused_classifier(head):
        return _norm_linear_parts(head.head) + _norm_linear_parts(head.head_dist)
    return None


def pack_head(weight, bias=None):
    """-> (wpack, bias32, key).  `weight` an nn.Linear's (K, C) weight with `bias` its (K) bias or None: wpack is the weight's own storage (float32,
    bfloat16 or float16, taken as it lies), bias32 the bias widened to float32.  `weight` an eval-mode, unfused RecNextClassifier (bias must be None):
    both BatchNorm1d folded and the two heads averaged in float32 (RecNextClassifier.fuse()'s arithmetic, once, in float32) into a float32 pack.
    key: address, version, dtype, device and shape of every tensor the pack was built from; a caller rebuilds the pack when it changes."""
    if isinstance(weight, torch.nn.Module):
        if bias is not None or not _is_unfused_classifier(weight):
            raise ValueError("pack_head takes a (K, C) weight with its bias, or an unfused RecNextClassifier (NormLinear heads of nn.BatchNorm1d + nn.Linear) alone")
        if weight.training:
            raise ValueError("pack_head folds running statistics: the RecNextClassifier must be in eval mode")
        parts = head_tensors(weight)
        with torch.no_grad():
            w32, b32 = fold_classifier(weight, torch.float32)
        return w32.contiguous(), b32.contiguous(), _key(parts)
    if not torch.is_tensor(weight) or weight.dim() != 2 or weight.dtype not in ops._DT or not weight.is_contiguous():
        raise ValueError("pack_head: weight must be a contiguous (K, C) tensor of float32, bfloat16 or float16")
    if bias is not None and (not torch.is_tensor(bias) or tuple(bias.shape) != (weight.shape[0],) or bias.device != weight.device):
        raise ValueError(f"pack_head: bias must be a ({weight.shape[0]},) tensor on {weight.device}")
    b32 = None if bias is None else bias.detach().to(torch.float32).contiguous()
    return weight.detach(), b32, _key([weight, bias])


def _check_x(fn, x):
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"{fn}: x must be a 4-D (N, C, H, W) tensor")
    if x.dtype not in ops._DT:
        raise ValueError(f"{fn}: x must be float32, bfloat16 or float16, got {x.dtype}")
    ops._require_gpu(x, "x")
    if 0 in x.shape:
        raise ValueError(f"{fn}: x has an empty extent: {tuple(x.shape)}")
    return ops._nhwc(x, "x")


def pool_head(x, wpack, bias, k):
    """head(x.mean((2, 3))) in one launch (rcx_pool_head_fwd): x N x C x H x W channels_last of float32 / bfloat16 / float16 -> (N, k) like x.  wpack:
    the contiguous (k, C) weight, float32 or of x's type (pack_head); bias float32 (k) or None."""
    x = _check_x("pool_head", x)
    n, c, h, w = x.shape
    k = int(k)
    if not torch.is_tensor(wpack) or wpack.dim() != 2 or tuple(wpack.shape) != (k, c) or wpack.dtype not in (torch.float32, x.dtype):
        raise ValueError(f"pool_head: wpack must be the ({k}, {c}) weight in float32 or {x.dtype} (pack_head)")
    ops._check_pack(wpack, wpack.dtype, k * c, x.device, "wpack")
    if bias is not None:
        ops._check_pack(bias, torch.float32, k, x.device, "bias")
    if not pool_head_supported(n, h, w, c, k, x.dtype, wpack.dtype):
        raise _lib.RcxError(f"pool_head: no kernel for N={n}, H={h}, W={w}, C={c}, K={k}, {x.dtype} with a {wpack.dtype} weight (pool_head_supported)")
    y = torch.empty((n, k), dtype=x.dtype, device=x.device)
    with ops._on(x.device):
        rc = _lib.load().rcx_pool_head_fwd(x.data_ptr(), wpack.data_ptr(), ptr(bias), y.data_ptr(), n, h, w, c, k,
                                           ops._dt(x), ops._DT[wpack.dtype], ops._stream(x.device))
    _lib.check(rc, "rcx_pool_head_fwd")
    return y


def global_pool(x):
    """x.mean((2, 3)) in one launch (rcx_global_pool_fwd): the float32 mean of every channel, rounded once: x N x C x H x W channels_last -> (N, C) like x."""
    x = _check_x("global_pool", x)
    n, c, h, w = x.shape
    if not pool_head_supported(n, h, w, c, 1, x.dtype):
        raise _lib.RcxError(f"global_pool: no kernel for N={n}, H={h}, W={w}, C={c}, {x.dtype} (pool_head_supported with K = 1)")
    y = torch.empty((n, c), dtype=x.dtype, device=x.device)
    with ops._on(x.device):
        rc = _lib.load().rcx_global_pool_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_global_pool_fwd")
    return y


class FusedHead:
    """``net.head(net.head_drop(x.mean((2, 3))))`` of an eval-mode RecNext (models.RecNext, lsmodels.RecNext and the share-channel models built on it) as
    ONE HIP launch (ops.pool_head; inference, channels_last, float32 / bfloat16 / float16).  Not a Module: it reads the head's own parameters and
    buffers (state_dict untouched) and rebuilds its pack when one of them changes.  ``net.head`` may be the nn.Linear replace_batchnorm leaves (the
    weight is taken as it lies) or an eval-mode unfused RecNextClassifier (folded and averaged in float32 at pack time); an nn.Identity head
    (``num_classes=0``) takes ops.global_pool."""

    def __init__(self, net, all_shapes=False):
        self.head = net.head
        self.all_shapes = bool(all_shapes)
        self._key, self._pack = None, None

    def _kind(self, net):
        head = net.head
        if head is not self.head:
            return None
        if type(head) is torch.nn.Linear:
            return "linear"
        if type(head) is torch.nn.Identity:
            return "identity"
        if _is_unfused_classifier(head) and not head.training and not head.head.norm.training and not head.head_dist.norm.training:
            return "classifier"
        return None

    def usable(self, net, x):
        """May this call take the HIP launch?  Only in eval mode with global_pool 'avg', when net.head is still the module that was attached and of a form
        the pack covers, x is a dense channels_last GPU tensor of a supported type, the head's parameters and buffers on its device and of its
        type, nothing on the way needs a gradient (ops.pool_head is a raw launch with no grad_fn), and a kernel exists for the shape -- and, unless
        all_shapes, the routing rule keeps it."""
        if net.training or net.global_pool != "avg":
            return False
        kind = self._kind(net)
        if kind is None or not torch.is_tensor(x) or x.dim() != 4 or not x.is_cuda or x.dtype not in ops._DT or 0 in x.shape:
            return False
        if not x.is_contiguous(memory_format=torch.channels_last) or x.data_ptr() % 16:
            return False                                # NCHW strides, or a view that starts off the 16 bytes the kernel's loads want
        n, c, h, w = x.shape
        parts = head_tensors(net.head) or []
        if any(t is not None and (t.device != x.device or t.dtype != x.dtype) for t in parts):
            return False                                # another device, or a type the module's own path would refuse or autocast would cast
        from .layers import _needs_grad
        if _needs_grad(x, *parts):
            return False
        if kind == "identity":
            k, wdtype = 1, x.dtype
        elif kind == "linear":
            wt = net.head.weight
            k, wdtype = wt.shape[0], wt.dtype
            if wt.dim() != 2 or wt.shape[1] != c or not wt.is_contiguous() or wt.data_ptr() % 16:
                return False
        else:
            lin = net.head.head.linear
            k, wdtype = lin.out_features, torch.float32
            if lin.in_features != c or net.head.head_dist.linear.in_features != c or net.head.head_dist.linear.out_features != k:
                return False
        return pool_head_supported(n, h, w, c, k, x.dtype, wdtype, measured_only=not self.all_shapes)

    def packs(self):
        return [] if self._pack is None else [p for p in self._pack if torch.is_tensor(p)]

    def _operands(self):
        head = self.head
        parts = head_tensors(head)
        key = _key(parts)
        if key != self._key:
            self._pack = pack_head(head.weight, head.bias)[:2] if type(head) is torch.nn.Linear else pack_head(head)[:2]
            self._key = key
        return self._pack

    def __call__(self, x):
        if type(self.head) is torch.nn.Identity:
            return global_pool(x)
        wpack, bias = self._operands()
        return pool_head(x, wpack, bias, wpack.shape[0])
