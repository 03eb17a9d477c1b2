"""RepVGGDW of a training step as one HIP operator (rcx_repdw_train_*, recnext_amd/csrc/rcx_repdw.hip; lsnet/model/recattn.py:8-15):
``r = lk.norm(lk.conv(x)) + sk.norm(sk.conv(x)) + x`` with both BatchNorms on batch statistics, three launches forward and at most four backward, one
autograd node, and x the only saved tensor of the activation's size.  ``lsmodels._rep_train`` calls ``RepDwFn`` for the modules
``models.use_fused_rep_train`` marked; everything else keeps the operator chain.

recnext_amd.ops exports the functions (``ops.repdw_train`` ...); why they are written here is said once, in recnext_amd/_trainop.py; their guard-band
cases are in tests/test_repdw_gpu.py.  A CPU tensor raises."""
import torch

from . import _lib, ops
from ._trainop import (carve_f32, check_dw_weight, check_like, check_rows, check_running, check_vec, check_x, esize, grad_in, grads_out, ptr, rows_routed,
                       supported, workspace)

# The routing rule (profiles/r21_rep_train.txt): (C, element size of x) -> the rows R = N H W at which the operator's forward +
# backward beat the operator chain by more than the chain's own spread at batch 128, in wall and in GPU time, in both jobs measured; from half the
# smallest such row count to twice the largest.  Left out: 128 channels at 28^2 and 56^2, 256 at 14^2 and 28^2, 384 at 14^2 (k_rep_bwd_dx is the
# slower there).  No timing at run time.
ROUTED = {(c, es): rows for c, rows in ((128, (12544, 50176)), (256, (3136, 12544)), (384, (3136, 12544)), (512, (1024, 12544))) for es in (2, 4)}


def repdw_train_routed(n, h, w, c, dtype):
    """Whether the routing rule keeps (N, H, W, C) of dtype on the fused operator: a rule on (R = N H W, C, element size) alone."""
    return rows_routed(ROUTED, (int(c), esize(dtype)), int(n) * int(h) * int(w))


def repdw_train_supported(n, h, w, c, dtype, measured_only=False):
    """Whether the kernels take (N, H, W, C) of dtype (rcx_repdw_train_supported: fewer than 2^31 elements; R = 1 is refused by the functions, as torch
    refuses it) and, with measured_only, the routing rule keeps it (repdw_train_routed)."""
    if dtype not in ops._DT or not supported("rcx_repdw_train_supported", n, h, w, c, ops._DT[dtype]):
        return False
    return not measured_only or repdw_train_routed(n, h, w, c, dtype)


def _check_params(fn, x, vecs, w3, w1):
    c = x.shape[1]
    for name, t in vecs:
        check_vec(fn, t, c, x.device, name)
    check_dw_weight(fn, w3, c, x.device, "w3", 3)
    check_dw_weight(fn, w1, c, x.device, "w1", 1)
    n, _, h, w = x.shape
    check_rows(n * h * w, tuple(x.shape))
    if not repdw_train_supported(n, h, w, c, x.dtype):
        raise ValueError(f"{fn}: no kernel for N={n}, H={h}, W={w}, C={c}, {x.dtype} (repdw_train_supported)")


def repdw_train(x, w3, b3, gamma_a, beta_a, w1, b1, gamma_b, beta_b, running=None, momentum_a=0.1, eps_a=1e-5, momentum_b=0.1, eps_b=1e-5):
    """RepVGGDW on batch statistics (rcx_repdw_train_fwd) on a dense channels_last x of float32 / bfloat16 / float16: w3 (C,1,3,3), b3 = lk.conv; gamma_a,
    beta_a, momentum_a, eps_a = lk.norm; w1 (C,1,1,1), b1 = sk.conv; gamma_b, beta_b, momentum_b, eps_b = sk.norm, all float32.  running: None or
    (lk running_mean, lk running_var, sk running_mean, sk running_var), updated in place.  -> (r float32 like x, stats float32 (4, C): mean x, var x,
    mean u, 1 / sqrt(var u + eps_a), u = lk.conv(x)), which repdw_train_backward takes."""
    fn = "repdw_train"
    check_x(fn, x)
    n, c, h, w = x.shape
    _check_params(fn, x, (("b3", b3), ("gamma_a", gamma_a), ("beta_a", beta_a), ("b1", b1), ("gamma_b", gamma_b), ("beta_b", beta_b)), w3, w1)
    run = check_running(fn, running, c, x.device, ("lk running_mean", "lk running_var", "sk running_mean", "sk running_var"))
    r = ops._empty_nhwc(n, c, h, w, torch.float32, x.device)
    stats = torch.empty((4, c), dtype=torch.float32, device=x.device)
    ws, nbytes = workspace("rcx_repdw_train_workspace_bytes", x.device, n, h, w, c, ops._DT[x.dtype])
    sp = stats.data_ptr()
    with ops._on(x.device):
        rc = _lib.load().rcx_repdw_train_fwd(x.data_ptr(), r.data_ptr(), w3.data_ptr(), b3.data_ptr(), gamma_a.data_ptr(), beta_a.data_ptr(), w1.data_ptr(),
                                             b1.data_ptr(), gamma_b.data_ptr(), beta_b.data_ptr(), run[0], run[1], run[2], run[3], sp, sp + 4 * c, sp + 8 * c,
                                             sp + 12 * c, ws.data_ptr(), nbytes, n, h, w, c, float(momentum_a), float(eps_a), float(momentum_b), float(eps_b),
                                             ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_repdw_train_fwd")
    return r, stats


GRADS = ("gw3", "gb3", "ggamma_a", "gbeta_a", "gw1", "gb1", "ggamma_b", "gbeta_b")


def repdw_train_backward(x, g, w3, b3, gamma_a, w1, gamma_b, stats, eps_b=1e-5, need_input_grad=True, need_param_grads=True):
    """Backward of repdw_train (rcx_repdw_train_bwd) from x and the forward's saved stats; g = dL/dr, float32, dense channels_last.
    -> (gx like x | None, grads | None), grads the float32 tuple GRADS: gw3 (C,1,3,3), gw1 (C,1,1,1), the rest (C); gb3 and gb1 are exact zeros."""
    fn = "repdw_train_backward"
    check_x(fn, x)
    check_like(fn, g, "g", x.shape, (torch.float32,), x.device)
    n, c, h, w = x.shape
    _check_params(fn, x, (("b3", b3), ("gamma_a", gamma_a), ("gamma_b", gamma_b)), w3, w1)
    if not torch.is_tensor(stats) or stats.dtype != torch.float32 or tuple(stats.shape) != (4, c) or stats.device != x.device or not stats.is_contiguous():
        raise ValueError(f"{fn}: stats must be the contiguous float32 (4, {c}) tensor repdw_train returned")
    if not (need_input_grad or need_param_grads):
        raise ValueError(f"{fn}: no gradient asked for")
    gx = ops._empty_nhwc(n, c, h, w, x.dtype, x.device) if need_input_grad else None
    grads, gp = None, [None] * 8
    if need_param_grads:
        grads, gp = carve_f32([(c, 1, 3, 3)] + [(c,)] * 3 + [(c, 1, 1, 1)] + [(c,)] * 3, x.device)        # GRADS: 16 C floats, one allocation
    ws, nbytes = workspace("rcx_repdw_train_workspace_bytes", x.device, n, h, w, c, ops._DT[x.dtype])
    sp = stats.data_ptr()
    with ops._on(x.device):
        rc = _lib.load().rcx_repdw_train_bwd(x.data_ptr(), g.data_ptr(), w3.data_ptr(), b3.data_ptr(), gamma_a.data_ptr(), w1.data_ptr(), gamma_b.data_ptr(),
                                             sp, sp + 4 * c, sp + 8 * c, sp + 12 * c, ptr(gx), *gp, ws.data_ptr(), nbytes,
                                             n, h, w, c, float(eps_b), ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_repdw_train_bwd")
    return gx, grads


class RepDwFn(torch.autograd.Function):
    """RepVGGDW on batch statistics with a HIP forward and backward: apply(x, w3, b3, gamma_a, beta_a, w1, b1, gamma_b, beta_b, lk_running_mean,
    lk_running_var, sk_running_mean, sk_running_var, momentum_a, eps_a, momentum_b, eps_b) -> r (float32).  The running buffers (all four or four
    None) are updated in place.  Saves x, the parameters the backward reads and the (4, C) statistics; once differentiable; the parameters' gradients
    come back in the parameters' dtype."""

    @staticmethod
    def forward(ctx, x, w3, b3, gamma_a, beta_a, w1, b1, gamma_b, beta_b, lk_rm, lk_rv, sk_rm, sk_rv, momentum_a, eps_a, momentum_b, eps_b):
        running = None if lk_rm is None else (lk_rm, lk_rv, sk_rm, sk_rv)
        r, stats = repdw_train(x, w3.detach(), b3.detach(), gamma_a.detach(), beta_a.detach(), w1.detach(), b1.detach(), gamma_b.detach(), beta_b.detach(),
                               running, momentum_a, eps_a, momentum_b, eps_b)
        ctx.save_for_backward(x, w3, b3, gamma_a, w1, gamma_b, stats)
        ctx.eps_b = eps_b
        return r

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w3, b3, gamma_a, w1, gamma_b, stats = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_x, need_p = need[0], any(need[1:9])
        if not (need_x or need_p):
            return (None,) * 17
        gx, grads = repdw_train_backward(x, grad_in(g, torch.float32), w3, b3, gamma_a, w1, gamma_b, stats, ctx.eps_b, need_input_grad=need_x,
                                         need_param_grads=need_p)
        f32 = torch.float32                                    # beta_a, b1 and beta_b are not saved: float32, as repdw_train took them
        return (gx, *grads_out(grads, (w3.dtype, b3.dtype, gamma_a.dtype, f32, w1.dtype, f32, gamma_b.dtype, f32), need[1:9]), *(None,) * 8)
