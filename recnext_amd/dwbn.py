"""A depthwise ConvNorm of a training step as one HIP operator (rcx_dwconv_bn_train_*, recnext_amd/csrc/rcx_dwbn.hip): the slice mixers' ``down[0]``
(5x5, stride 2), ``pe`` (3x3), ``conv`` (5x5 on ``x + resize(a)``) and ``LinearAttention3.pe`` (lsnet/model/recattn.py:54-67, :89-112),
``y = norm(conv(z))`` with the BatchNorm on batch statistics: three launches forward and at most five backward, one autograd node, and x, a and the
conv's float32 output u the saved activations (the count of the operator chain: x, a and the BatchNorm's input).  ``recattn._conv_norm_train`` and
``_upadd_conv_norm_train`` call ``DwConvBnFn`` for the modules ``models.use_fused_conv_norm_train`` marked; everything else keeps the operator chain.

recnext_amd.ops exports the functions (``ops.dwconv_bn_train`` ...); why they are written here is said once, in recnext_amd/_trainop.py; their
guard-band cases are in tests/test_conv_norm_gpu.py.  A CPU tensor raises."""
import torch

from . import _lib, ops
from ._trainop import (carve_f32, check_dw_weight, check_like, check_rows, check_running, check_vec, check_x, dense_nhwc, esize, grad_in, grads_out, ptr,
                       rows_routed, supported, workspace)

# The routing rule (profiles/r24_conv_norm_train.txt): (C, k, stride, has_coarse, element size of x) -> the output rows
# R = N Ho Wo at which the operator's forward + backward beat the operator chain by more than the chain's own spread at batch 128, in wall and in GPU
# time, in both jobs measured; from half the smallest such row count to twice the largest.  No timing at run time.  A shape that is not here stays on
# the chain.  Left out: every up-add shape (the 5x5 conv on x + resize(a): 0.35 - 0.8 x, k_dwbn_stats and k_dwbn_bwd_dx_up are the slower there), the
# stride-2 5x5 at 32 x 28^2, 64 x 28^2 and 32 x 56^2, the 3x3 at 32 x 28^2 and at 128 x 7^2 (LinearAttention3's: a win in one job, inside the chain's
# spread in the other), and the element sizes missing below (a win in one job only).
ROUTED = {(32, 3, 1, False, 4): (12544, 50176), (64, 3, 1, False, 4): (3136, 50176), (64, 3, 1, False, 2): (12544, 50176), (64, 5, 2, False, 2): (3136, 12544),
          (96, 5, 2, False, 4): (3136, 12544), (96, 5, 2, False, 2): (3136, 12544), (96, 3, 1, False, 4): (3136, 12544), (96, 3, 1, False, 2): (3136, 12544)}


def dwconv_bn_train_routed(n, h, w, c, k, stride, has_coarse, dtype):
    """Whether the routing rule keeps the shape on the fused operator: a rule on (R = N Ho Wo, C, k, stride, has_coarse, element size) alone."""
    ho, wo = _out_hw(int(h), int(w), int(stride))
    return rows_routed(ROUTED, (int(c), int(k), int(stride), bool(has_coarse), esize(dtype)), int(n) * ho * wo)


def dwconv_bn_train_supported(n, h, w, c, k, stride, has_coarse, dtype, measured_only=False):
    """Whether the kernels take x of (N, H, W, C) and dtype with a k x k conv of this stride (rcx_dwconv_bn_train_supported: k 3 or 5, stride 1 or 2, the
    up-add form at stride 1, fewer than 2^31 elements; one output value a channel is refused by the functions, as torch refuses it) and, with
    measured_only, the routing rule keeps it (dwconv_bn_train_routed)."""
    if dtype not in ops._DT or not supported("rcx_dwconv_bn_train_supported", n, h, w, c, k, stride, bool(has_coarse), ops._DT[dtype]):
        return False
    return not measured_only or dwconv_bn_train_routed(n, h, w, c, k, stride, has_coarse, dtype)


def _out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def _check(fn, x, w, a, stride, vecs):
    """-> (k, Ho, Wo, Hc, Wc) after the checks every entry shares."""
    check_x(fn, x)
    n, c, h, wd = x.shape
    for name, t in vecs:
        if t is not None:
            check_vec(fn, t, c, x.device, name)
    k = check_dw_weight(fn, w, c, x.device, "w")
    hc = wc = 0
    if a is not None:
        check_x(fn, a, "a")
        if a.dtype != torch.float32 or a.shape[0] != n or a.shape[1] != c or a.device != x.device:
            raise ValueError(f"{fn}: a is {tuple(a.shape)} {a.dtype} on {a.device}, wanted float32 ({n}, {c}, Hc, Wc) on {x.device}")
        hc, wc = a.shape[2], a.shape[3]
    ho, wo = _out_hw(h, wd, stride) if stride in (1, 2) else (0, 0)
    check_rows(n * ho * wo, (n, c, ho, wo))
    if not dwconv_bn_train_supported(n, h, wd, c, k, stride, a is not None, x.dtype):
        raise ValueError(f"{fn}: no kernel for N={n}, H={h}, W={wd}, C={c}, k={k}, stride={stride}, {'up-add, ' if a is not None else ''}{x.dtype} "
                         "(dwconv_bn_train_supported)")
    return k, ho, wo, hc, wc


def dwconv_bn_train(x, w, b, gamma, beta, a=None, stride=1, running=None, momentum=0.1, eps=1e-5):
    """norm(conv(z)) on batch statistics (rcx_dwconv_bn_train_fwd) on a dense channels_last x of float32 / bfloat16 / float16: z = x, or, with a (float32,
    dense channels_last, (N, C, Hc, Wc); stride 1), z = x + nearest-resize(a); w (C,1,k,k), k 3 or 5, b (C) or None = the conv; gamma, beta, momentum,
    eps = the norm, all float32.  running: None or (running_mean, running_var), updated in place.  -> (y like x at the output size, stats float32 (2, C):
    mean u and 1 / sqrt(var u + eps), u float32 like y: the conv's output), the last two for dwconv_bn_train_backward."""
    fn = "dwconv_bn_train"
    k, ho, wo, hc, wc = _check(fn, x, w, a, stride, (("b", b), ("gamma", gamma), ("beta", beta)))
    n, c, h, wd = x.shape
    run = check_running(fn, running, c, x.device, ("running_mean", "running_var"))
    y = ops._empty_nhwc(n, c, ho, wo, x.dtype, x.device)
    u = ops._empty_nhwc(n, c, ho, wo, torch.float32, x.device)
    stats = torch.empty((2, c), dtype=torch.float32, device=x.device)
    ws, nbytes = workspace("rcx_dwconv_bn_train_workspace_bytes", x.device, n, h, wd, c, k, stride, int(a is not None), ops._DT[x.dtype])
    sp = stats.data_ptr()
    with ops._on(x.device):
        rc = _lib.load().rcx_dwconv_bn_train_fwd(x.data_ptr(), ptr(a), hc, wc, w.data_ptr(), ptr(b), gamma.data_ptr(), beta.data_ptr(), run[0], run[1],
                                                 y.data_ptr(), u.data_ptr(), sp, sp + 4 * c, ws.data_ptr(), nbytes, n, h, wd, c, k, int(stride),
                                                 float(momentum), float(eps), ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_dwconv_bn_train_fwd")
    return y, stats, u


GRADS = ("gw", "gb", "ggamma", "gbeta")


def dwconv_bn_train_backward(x, g, w, gamma, stats, u, a=None, stride=1, need_input_grad=True, need_coarse_grad=None, need_param_grads=True):
    """Backward of dwconv_bn_train (rcx_dwconv_bn_train_bwd) from x, a, the forward's stats and u; g = dL/dy in y's dtype, dense channels_last.
    need_coarse_grad defaults to whether a is given.  -> (gx like x | None, ga float32 like a | None, grads | None), grads the float32 tuple GRADS:
    gw (C,1,k,k), the rest (C); gb is exact zeros (a bias in front of a BatchNorm on batch statistics has no gradient)."""
    fn = "dwconv_bn_train_backward"
    k, ho, wo, hc, wc = _check(fn, x, w, a, stride, (("gamma", gamma),))
    n, c, h, wd = x.shape
    need_coarse_grad = (a is not None) if need_coarse_grad is None else bool(need_coarse_grad)
    if need_coarse_grad and a is None:
        raise ValueError(f"{fn}: need_coarse_grad without a")
    check_like(fn, g, "g", (n, c, ho, wo), (x.dtype,), x.device)
    if not torch.is_tensor(u) or u.dim() != 4 or tuple(u.shape) != (n, c, ho, wo) or u.dtype != torch.float32 or u.device != x.device or not dense_nhwc(u):
        raise ValueError(f"{fn}: u must be the dense channels_last float32 {(n, c, ho, wo)} tensor dwconv_bn_train returned")
    if not torch.is_tensor(stats) or stats.dtype != torch.float32 or tuple(stats.shape) != (2, c) or stats.device != x.device or not stats.is_contiguous():
        raise ValueError(f"{fn}: stats must be the contiguous float32 (2, {c}) tensor dwconv_bn_train returned")
    if not (need_input_grad or need_coarse_grad or need_param_grads):
        raise ValueError(f"{fn}: no gradient asked for")
    gx = ops._empty_nhwc(n, c, h, wd, x.dtype, x.device) if need_input_grad else None
    ga = ops._empty_nhwc(n, c, hc, wc, torch.float32, x.device) if need_coarse_grad else None
    grads, gp = None, [None] * 4
    if need_param_grads:
        grads, gp = carve_f32([(c, 1, k, k)] + [(c,)] * 3, x.device)                  # GRADS: (k k + 3) C floats, one allocation
    ws, nbytes = workspace("rcx_dwconv_bn_train_workspace_bytes", x.device, n, h, wd, c, k, stride, int(a is not None), ops._DT[x.dtype])
    sp = stats.data_ptr()
    with ops._on(x.device):
        rc = _lib.load().rcx_dwconv_bn_train_bwd(x.data_ptr(), ptr(a), hc, wc, u.data_ptr(), g.data_ptr(), w.data_ptr(), gamma.data_ptr(), sp, sp + 4 * c,
                                                 ptr(gx), ptr(ga), *gp, ws.data_ptr(), nbytes, n, h, wd, c, k, int(stride), ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_dwconv_bn_train_bwd")
    return gx, ga, grads


class DwConvBnFn(torch.autograd.Function):
    """A depthwise ConvNorm on batch statistics with a HIP forward and backward: apply(x, a, w, b, gamma, beta, running_mean, running_var, stride,
    momentum, eps) -> y in x's dtype.  a (the coarse plane of the up-add form, any float dtype; taken in float32) and b may be None; the running
    buffers (both or two None) are updated in place.  Saves x, a, w, gamma, the (2, C) statistics and the conv's float32 output; once differentiable;
    the parameters' gradients come back in the parameters' dtype, a's in a's."""

    @staticmethod
    def forward(ctx, x, a, w, b, gamma, beta, running_mean, running_var, stride, momentum, eps):
        running = None if running_mean is None else (running_mean, running_var)
        a32 = None if a is None else ops._nhwc(a.detach() if a.dtype == torch.float32 else a.detach().float(), "a")
        y, stats, u = dwconv_bn_train(x, w.detach(), None if b is None else b.detach(), gamma.detach(), beta.detach(), a32, stride, running, momentum, eps)
        ctx.save_for_backward(x, a32, w, gamma, stats, u)
        ctx.stride, ctx.adtype, ctx.bdtype, ctx.betadtype = stride, None if a is None else a.dtype, None if b is None else b.dtype, beta.dtype
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, a32, w, gamma, stats, u = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_x, need_a, need_p = need[0], a32 is not None and need[1], any(need[2:6])
        if not (need_x or need_a or need_p):
            return (None,) * 11
        gx, ga, grads = dwconv_bn_train_backward(x, grad_in(g, x.dtype), w, gamma, stats, u, a32, ctx.stride, need_input_grad=need_x, need_coarse_grad=need_a,
                                                 need_param_grads=need_p)
        if ga is not None and ga.dtype != ctx.adtype:
            ga = ga.to(ctx.adtype)
        return (gx, ga, *grads_out(grads, (w.dtype, ctx.bdtype, gamma.dtype, ctx.betadtype), need[2:6]), *(None,) * 5)
