"""nn.BatchNorm2d of a training step on HIP (rcx_batchnorm_*, recnext_amd/csrc/rcx_bn.hip): batch statistics and apply, the frozen-statistics apply,
their backward, the autograd Function and the module that routes to them.  Every BatchNorm of a training step is the module's own nn.BatchNorm2d called
on a dense channels_last tensor (``m.norm(...)`` in recattn._conv_norm_train, lsmodels._rep_train, the ConvNorms of the channel mixers,
MetaNeXtBlock.norm / Downsample.norm), so one operator swapped in at module level (``models.use_hip_batchnorm``) reaches all of them.

recnext_amd.ops exports the functions (``ops.batch_norm_train`` ...); they are written here because tests/test_guard_cpu.py asks a row in the case table
of tests/test_guard_bands_gpu.py of every launching function whose source is in ops.py, and these entries' guard-band cases are in
tests/test_batchnorm_gpu.py, which passes this module to tests/guard.py as one of ``modules=`` (as recnext_amd/lsdown.py does): outputs, statistics,
gradients and the workspace are allocated by this module's own ``torch.empty``.  A CPU tensor raises in the functions; only ``HipBatchNorm2d`` has a
fallback, and that is its parent's forward, unchanged."""
import torch
import torch.nn as nn

from . import _lib, ops


# The routing rule (profiles/r20_batchnorm.txt): the (C, 16-bit | float32) whose forward + backward beat the library's BatchNorm by
# more than the library's own spread at batch 128, each with the rows R = N H W from half to twice the measured count.  No timing at run time.
ROUTED = {(128, 2): (50176, 200704), (256, 2): (12544, 50176), (256, 4): (12544, 50176), (768, 2): (3136, 12544)}


def batch_norm_routed(n, h, w, c, dtype):
    """Whether the routing rule keeps (N, H, W, C) of dtype on the HIP BatchNorm: a rule on (R = N H W, C, element size) alone."""
    lo, hi = ROUTED.get((int(c), 4 if dtype == torch.float32 else 2), (1, 0))
    return lo <= int(n) * int(h) * int(w) <= hi


def batch_norm_supported(n, h, w, c, dtype, measured_only=True):
    """Whether HipBatchNorm2d routes (N, H, W, C) of dtype to rcx_batchnorm_*: the kernels take it (rcx_batchnorm_supported: fewer than 2^31 elements)
    and, unless measured_only is False, the routing rule keeps it (batch_norm_routed).  The functions below run every shape the kernels take."""
    if dtype not in ops._DT or _lib.load().rcx_batchnorm_supported(int(n), int(h), int(w), int(c), ops._DT[dtype]) <= 0:
        return False
    return not measured_only or batch_norm_routed(n, h, w, c, dtype)


def _dense_nhwc(t):
    n, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    return all(sz == 1 or st == wt for sz, st, wt in zip(t.shape, t.stride(), want))


def _check_x(fn, x, name="x"):
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"{fn}: {name} must be a 4-D (N, C, H, W) tensor")
    if x.dtype not in ops._DT:
        raise ValueError(f"{fn}: {name} must be float32, bfloat16 or float16, got {x.dtype}")
    ops._require_gpu(x, name)
    if x.numel() == 0:
        raise ValueError(f"{fn}: {name} is empty, shape {tuple(x.shape)}")
    if not _dense_nhwc(x):
        raise ValueError(f"{fn}: {name} must be dense channels_last (N x H x W x C storage), got shape {tuple(x.shape)} strides {x.stride()}")


def _check_vec(fn, t, c, device, name):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (c,) or t.device != device or not t.is_contiguous():
        raise ValueError(f"{fn}: {name} must be a contiguous float32 ({c},) tensor on {device}")


def _supported_or_raise(fn, x):
    n, c, h, w = x.shape
    if not batch_norm_supported(n, h, w, c, x.dtype, measured_only=False):
        raise ValueError(f"{fn}: no kernel for N={n}, H={h}, W={w}, C={c}, {x.dtype} (batch_norm_supported)")


def _workspace(x):
    n, c, h, w = x.shape
    nbytes = _lib.load().rcx_batchnorm_workspace_bytes(n, h, w, c, ops._DT[x.dtype])
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device), nbytes


def batch_norm_train(x, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """F.batch_norm(x, running_mean, running_var, weight, bias, training=True, momentum, eps) on a dense channels_last x (rcx_batchnorm_train_fwd):
    -> (y like x, save_mean, save_invstd), the statistics float32 (C).  running_mean / running_var (both or neither) are updated in place."""
    fn = "batch_norm_train"
    _check_x(fn, x)
    n, c, h, w = x.shape
    _check_vec(fn, weight, c, x.device, "weight")
    _check_vec(fn, bias, c, x.device, "bias")
    if (running_mean is None) != (running_var is None):
        raise ValueError(f"{fn}: running_mean and running_var come together or not at all")
    if running_mean is not None:
        _check_vec(fn, running_mean, c, x.device, "running_mean")
        _check_vec(fn, running_var, c, x.device, "running_var")
    if n * h * w == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    _supported_or_raise(fn, x)
    y = torch.empty((n, h, w, c), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2)
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    invstd = torch.empty(c, dtype=torch.float32, device=x.device)
    ws, nbytes = _workspace(x)
    ptr = lambda t: t.data_ptr() if t is not None else None
    with ops._on(x.device):
        rc = _lib.load().rcx_batchnorm_train_fwd(x.data_ptr(), y.data_ptr(), weight.data_ptr(), bias.data_ptr(), ptr(running_mean), ptr(running_var),
                                                 mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nbytes, n, h, w, c, float(momentum), float(eps),
                                                 ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_batchnorm_train_fwd")
    return y, mean, invstd


def batch_norm_frozen(x, weight, bias, mean, var, eps=1e-5):
    """Eval-mode BatchNorm (given statistics) on a dense channels_last x in one launch (rcx_batchnorm_frozen_fwd): -> (y like x, invstd), invstd the
    float32 (C) 1 / sqrt(var + eps) the kernel used, which batch_norm_backward takes."""
    fn = "batch_norm_frozen"
    _check_x(fn, x)
    n, c, h, w = x.shape
    for name, t in (("weight", weight), ("bias", bias), ("mean", mean), ("var", var)):
        _check_vec(fn, t, c, x.device, name)
    _supported_or_raise(fn, x)
    y = torch.empty((n, h, w, c), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2)
    invstd = torch.empty(c, dtype=torch.float32, device=x.device)
    with ops._on(x.device):
        rc = _lib.load().rcx_batchnorm_frozen_fwd(x.data_ptr(), y.data_ptr(), weight.data_ptr(), bias.data_ptr(), mean.data_ptr(), var.data_ptr(),
                                                  invstd.data_ptr(), float(eps), n, h, w, c, ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_batchnorm_frozen_fwd")
    return y, invstd


def batch_norm_backward(x, gy, weight, mean, invstd, batch_stats=True, need_input_grad=True, need_param_grads=True):
    """Backward of batch_norm_train (batch_stats) / batch_norm_frozen (rcx_batchnorm_bwd) from the forward's saved float32 mean and invstd:
    -> (gx like x | None, gweight float32 (C) | None, gbias float32 (C) | None).  gy has x's dtype and layout."""
    fn = "batch_norm_backward"
    _check_x(fn, x)
    _check_x(fn, gy, "gy")
    if gy.shape != x.shape or gy.dtype != x.dtype or gy.device != x.device:
        raise ValueError(f"{fn}: gy is {tuple(gy.shape)} {gy.dtype} on {gy.device}, x {tuple(x.shape)} {x.dtype} on {x.device}")
    n, c, h, w = x.shape
    for name, t in (("weight", weight), ("mean", mean), ("invstd", invstd)):
        _check_vec(fn, t, c, x.device, name)
    if not (need_input_grad or need_param_grads):
        raise ValueError(f"{fn}: no gradient asked for")
    if batch_stats and n * h * w == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    _supported_or_raise(fn, x)
    gx = torch.empty((n, h, w, c), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2) if need_input_grad else None
    gw = torch.empty(c, dtype=torch.float32, device=x.device) if need_param_grads else None
    gb = torch.empty(c, dtype=torch.float32, device=x.device) if need_param_grads else None
    ws, nbytes = _workspace(x) if (batch_stats or need_param_grads) else (None, 0)
    ptr = lambda t: t.data_ptr() if t is not None else None
    with ops._on(x.device):
        rc = _lib.load().rcx_batchnorm_bwd(x.data_ptr(), gy.data_ptr(), weight.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ptr(gx), ptr(gw), ptr(gb),
                                           ptr(ws), nbytes, n, h, w, c, 1 if batch_stats else 0, ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_batchnorm_bwd")
    return gx, gw, gb


class BatchNormFn(torch.autograd.Function):
    """BatchNorm2d with a HIP forward and backward.  training: batch statistics (running_mean / running_var updated in place when given); else the given
    running statistics, frozen.  Saves x, weight, mean and invstd and nothing else; the parameters' gradients come back in the parameters' dtype."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps):
        if training:
            y, mean, invstd = batch_norm_train(x, weight.detach(), bias.detach(), running_mean, running_var, momentum, eps)
        else:
            mean = running_mean
            y, invstd = batch_norm_frozen(x, weight.detach(), bias.detach(), running_mean, running_var, eps)
        ctx.save_for_backward(x, weight, mean, invstd)
        ctx.batch_stats = bool(training)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, mean, invstd = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (need_x or need_p):
            return (None,) * 8
        if gy.dtype != x.dtype:
            gy = gy.to(x.dtype)
        if not _dense_nhwc(gy):
            gy = ops._nhwc(gy, "gy")
        gx, gw, gb = batch_norm_backward(x, gy, weight.detach(), mean, invstd, ctx.batch_stats, need_input_grad=need_x, need_param_grads=need_p)
        return (gx, gw.to(weight.dtype) if ctx.needs_input_grad[1] else None, gb.to(weight.dtype) if ctx.needs_input_grad[2] else None,
                None, None, None, None, None)


class HipBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d (same parameters, buffers and state_dict keys) whose forward runs on the HIP kernels when it can: a GPU tensor, 4-D, dense
    channels_last, float32 / bfloat16 / float16, affine with float32 weight and bias, float32 running buffers (or none), a float momentum, a shape
    batch_norm_supported takes (the routing rule; every shape the kernels take when ``hip_all_shapes`` is set), and either training mode or eval mode with something wanting a gradient (the frozen-statistics backbone).  Everything
    else -- eval under no_grad, CPU, NCHW-strided input, 16-bit parameters, momentum=None -- is nn.BatchNorm2d.forward, unchanged to the bit."""

    hip_all_shapes = False            # set per module by models.use_hip_batchnorm(net, all_shapes=True): route whatever the kernels take

    def _hip_ok(self, x):
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in ops._DT and x.numel() > 0):
            return False
        w, b = self.weight, self.bias
        if w is None or b is None or w.dtype != torch.float32 or b.dtype != torch.float32 or not isinstance(self.momentum, float):
            return False
        rm, rv = self.running_mean, self.running_var
        if (rm is None) != (rv is None) or (rm is not None and (rm.dtype != torch.float32 or rv.dtype != torch.float32)):
            return False
        if self.training or rm is None:
            mode_ok = True                                               # batch statistics (no running buffers: in eval mode too, as the parent)
        else:
            mode_ok = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad)
        if not mode_ok or not _dense_nhwc(x):
            return False
        n, c, h, wd = x.shape
        return c == self.num_features and w.device == x.device and batch_norm_supported(n, h, wd, c, x.dtype, measured_only=not self.hip_all_shapes)

    def forward(self, x):
        if not self._hip_ok(x):
            return super().forward(x)
        batch = self.training or self.running_mean is None
        if batch and x.numel() // x.shape[1] == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")
        track = self.training and self.track_running_stats and self.running_mean is not None
        if track and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
        return BatchNormFn.apply(x, self.weight, self.bias, self.running_mean if (track or not batch) else None,
                                 self.running_var if (track or not batch) else None, batch, self.momentum, self.eps)
