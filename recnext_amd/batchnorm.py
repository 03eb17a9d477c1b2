"""nn.BatchNorm2d of a training step on HIP (rcx_batchnorm_*, recnext_amd/csrc/rcx_bn.hip): batch statistics and apply, the frozen-statistics apply,
their backward, the autograd Function and the module that routes to them.  Every BatchNorm of a training step is the module's own nn.BatchNorm2d called
on a dense channels_last tensor (``m.norm(...)`` in recattn._conv_norm_train, lsmodels._rep_train, the ConvNorms of the channel mixers,
MetaNeXtBlock.norm / Downsample.norm), so one operator swapped in at module level (``models.use_hip_batchnorm``) reaches all of them.

recnext_amd.ops exports the functions (``ops.batch_norm_train`` ...); why they are written here is said once, in recnext_amd/_trainop.py; their
guard-band cases are in tests/test_batchnorm_gpu.py.  A CPU tensor raises in the functions; only ``HipBatchNorm2d`` has a fallback, and that is its
parent's forward, unchanged.  ``norm_fusable`` and ``bump`` are what the operators that take a module's BatchNorm over (repdw.py, dwbn.py, bnact.py)
ask of it."""
import torch
import torch.nn as nn

from . import _lib, ops
from ._trainop import (check_like, check_rows, check_running, check_vec, check_x, esize, gpu_tensor_ok, grad_in, grads_out, ptr, rows_routed, supported,
                       workspace)
from ._trainop import dense_nhwc as _dense_nhwc          # the tests ask it of the outputs under this name


# The routing rule (profiles/r20_batchnorm.txt): the (C, 16-bit | float32) whose forward + backward beat the library's BatchNorm by
# more than the library's own spread at batch 128, each with the rows R = N H W from half to twice the measured count.  No timing at run time.
ROUTED = {(128, 2): (50176, 200704), (256, 2): (12544, 50176), (256, 4): (12544, 50176), (768, 2): (3136, 12544)}


def batch_norm_routed(n, h, w, c, dtype):
    """Whether the routing rule keeps (N, H, W, C) of dtype on the HIP BatchNorm: a rule on (R = N H W, C, element size) alone."""
    return rows_routed(ROUTED, (int(c), esize(dtype)), int(n) * int(h) * int(w))


def batch_norm_supported(n, h, w, c, dtype, measured_only=True):
    """Whether HipBatchNorm2d routes (N, H, W, C) of dtype to rcx_batchnorm_*: the kernels take it (rcx_batchnorm_supported: fewer than 2^31 elements)
    and, unless measured_only is False, the routing rule keeps it (batch_norm_routed).  The functions below run every shape the kernels take."""
    if dtype not in ops._DT or not supported("rcx_batchnorm_supported", n, h, w, c, ops._DT[dtype]):
        return False
    return not measured_only or batch_norm_routed(n, h, w, c, dtype)


def _supported_or_raise(fn, x):
    n, c, h, w = x.shape
    if not batch_norm_supported(n, h, w, c, x.dtype, measured_only=False):
        raise ValueError(f"{fn}: no kernel for N={n}, H={h}, W={w}, C={c}, {x.dtype} (batch_norm_supported)")


def batch_norm_train(x, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """F.batch_norm(x, running_mean, running_var, weight, bias, training=True, momentum, eps) on a dense channels_last x (rcx_batchnorm_train_fwd):
    -> (y like x, save_mean, save_invstd), the statistics float32 (C).  running_mean / running_var (both or neither) are updated in place."""
    fn = "batch_norm_train"
    check_x(fn, x)
    n, c, h, w = x.shape
    check_vec(fn, weight, c, x.device, "weight")
    check_vec(fn, bias, c, x.device, "bias")
    run = check_running(fn, (running_mean, running_var), c, x.device, ("running_mean", "running_var"))
    check_rows(n * h * w, tuple(x.shape))
    _supported_or_raise(fn, x)
    y = ops._empty_nhwc(n, c, h, w, x.dtype, x.device)
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    invstd = torch.empty(c, dtype=torch.float32, device=x.device)
    ws, nbytes = workspace("rcx_batchnorm_workspace_bytes", x.device, n, h, w, c, ops._DT[x.dtype])
    with ops._on(x.device):
        rc = _lib.load().rcx_batchnorm_train_fwd(x.data_ptr(), y.data_ptr(), weight.data_ptr(), bias.data_ptr(), run[0], run[1],
                                                 mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nbytes, n, h, w, c, float(momentum), float(eps),
                                                 ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_batchnorm_train_fwd")
    return y, mean, invstd


def batch_norm_frozen(x, weight, bias, mean, var, eps=1e-5):
    """Eval-mode BatchNorm (given statistics) on a dense channels_last x in one launch (rcx_batchnorm_frozen_fwd): -> (y like x, invstd), invstd the
    float32 (C) 1 / sqrt(var + eps) the kernel used, which batch_norm_backward takes."""
    fn = "batch_norm_frozen"
    check_x(fn, x)
    n, c, h, w = x.shape
    for name, t in (("weight", weight), ("bias", bias), ("mean", mean), ("var", var)):
        check_vec(fn, t, c, x.device, name)
    _supported_or_raise(fn, x)
    y = ops._empty_nhwc(n, c, h, w, x.dtype, x.device)
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
    check_x(fn, x)
    check_like(fn, gy, "gy", x.shape, (x.dtype,), x.device)
    n, c, h, w = x.shape
    for name, t in (("weight", weight), ("mean", mean), ("invstd", invstd)):
        check_vec(fn, t, c, x.device, name)
    if not (need_input_grad or need_param_grads):
        raise ValueError(f"{fn}: no gradient asked for")
    if batch_stats:
        check_rows(n * h * w, tuple(x.shape))
    _supported_or_raise(fn, x)
    gx = ops._empty_nhwc(n, c, h, w, x.dtype, x.device) if need_input_grad else None
    gw = torch.empty(c, dtype=torch.float32, device=x.device) if need_param_grads else None
    gb = torch.empty(c, dtype=torch.float32, device=x.device) if need_param_grads else None
    ws, nbytes = None, 0
    if batch_stats or need_param_grads:
        ws, nbytes = workspace("rcx_batchnorm_workspace_bytes", x.device, n, h, w, c, ops._DT[x.dtype])
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
        gx, gw, gb = batch_norm_backward(x, grad_in(gy, x.dtype, "gy"), weight.detach(), mean, invstd, ctx.batch_stats, need_input_grad=need_x,
                                         need_param_grads=need_p)
        return (gx, *grads_out((gw, gb), (weight.dtype, weight.dtype), ctx.needs_input_grad[1:3]), None, None, None, None, None)


def _params_ok(bn):
    """The parameters and buffers the kernels take: affine with float32 weight and bias, float32 running buffers or none, a float momentum."""
    w, b, rm, rv = bn.weight, bn.bias, bn.running_mean, bn.running_var
    if w is None or b is None or w.dtype != torch.float32 or b.dtype != torch.float32 or not isinstance(bn.momentum, float):
        return False
    return (rm is None) == (rv is None) and (rm is None or (rm.dtype == torch.float32 and rv.dtype == torch.float32))


def norm_fusable(bn):
    """A BatchNorm an operator that takes it over reproduces: exactly nn.BatchNorm2d or HipBatchNorm2d, in training mode, with _params_ok."""
    return type(bn) in (nn.BatchNorm2d, HipBatchNorm2d) and bn.training and _params_ok(bn)


def bump(bn):
    """What nn.BatchNorm2d.forward does before a training call that updates the running buffers: num_batches_tracked += 1.
    -> (running_mean, running_var) for the operator to update in place, or (None, None) when the norm has none."""
    if bn.running_mean is None:
        return None, None
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return bn.running_mean, bn.running_var


class HipBatchNorm2d(nn.BatchNorm2d):
    """nn.BatchNorm2d (same parameters, buffers and state_dict keys) whose forward runs on the HIP kernels when it can: a GPU tensor, 4-D, dense
    channels_last, float32 / bfloat16 / float16, affine with float32 weight and bias, float32 running buffers (or none), a float momentum, a shape
    batch_norm_supported takes (the routing rule; every shape the kernels take when ``hip_all_shapes`` is set), and either training mode or eval mode with something wanting a gradient (the frozen-statistics backbone).  Everything
    else -- eval under no_grad, CPU, NCHW-strided input, 16-bit parameters, momentum=None -- is nn.BatchNorm2d.forward, unchanged to the bit."""

    hip_all_shapes = False            # set per module by models.use_hip_batchnorm(net, all_shapes=True): route whatever the kernels take

    def _hip_ok(self, x):
        if not (gpu_tensor_ok(x) and x.numel() > 0 and _params_ok(self)):
            return False
        w, b, rm = self.weight, self.bias, self.running_mean
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
        if batch:
            check_rows(x.numel() // x.shape[1], x.size())
        track = self.training and self.track_running_stats and self.running_mean is not None
        if track and self.num_batches_tracked is not None:
            self.num_batches_tracked.add_(1)
        return BatchNormFn.apply(x, self.weight, self.bias, self.running_mean if (track or not batch) else None,
                                 self.running_var if (track or not batch) else None, batch, self.momentum, self.eps)
