"""The two BatchNorms of a channel mixer in a training step with what follows them as an epilogue (rcx_bn_act_*, recnext_amd/csrc/rcx_bnact.hip):
``bn_gelu`` = ``GELU(BN(u))`` on batch statistics, which saves u and the (C) statistics and never holds ``BN(u)``, and ``bn_add`` = ``r + s[n] BN(u)``,
the residual add behind the mixer with the optional per-sample DropPath scale.  ``models.use_fused_mixer_norms_train`` marks the channel mixers
(lsnet/model/recattn.py:199-205, :240-263; model/recnext.py:125-171) and the stems (:208-223; :134-146); ``run_mixer`` / ``run_stem`` below are what the
marked modules' forwards call, and everything they do not route is the operator chain, unchanged to the bit.

recnext_amd.ops exports the functions (``ops.bn_gelu_train`` ...); why they are written here is said once, in recnext_amd/_trainop.py; their
guard-band cases are in tests/test_bnact_gpu.py.  A CPU tensor raises."""
import torch
import torch.nn as nn

from . import _lib, ops
from ._trainop import (check_like, check_rows, check_running, check_vec, check_x, esize, gpu_tensor_ok, grad_in, grads_out, ptr, rows_routed, supported,
                       workspace)
from .batchnorm import bump, norm_fusable
from .layers import ConvNorm, DropPath, _is_exact_gelu

EPILOGUES = {"gelu": 0, "add": 1}                  # RCX_BN_EPI_GELU, RCX_BN_EPI_ADD
ATTR = "_fused_mixer_norms_train"

# The routing rule (profiles/r26_mixer_norms_train.txt): (C, element size of u, epilogue) -> the rows R = N H W at which the
# operator's forward + backward beat the operator chain at batch 128 by more than the chain's own spread in that job AND by at least a tenth, in wall
# and in GPU time, in each of the two jobs measured; from half to twice the measured rows (the rule of section 5.z).  No timing at run time.  A shape
# that is not here stays on the chain.  The tenth: a call of the operator costs the host some 94 us forward + backward where the chain costs it
# 80 - 90, so a smaller win of the isolated call is a loss in a host-bound step (recnext_t with every shape routed: + 3.4 ms a step).  No ADD row is
# here: each won in the first job (1.05 - 1.6 x) and all but one missed the rule in the second, on a busy host, and the key does not tell the
# residual's type apart.  GELU rows that won the first job and not the second (inside the chain's spread there, or slower): (64, 100352) and
# (256, 25088) in 16-bit, (256, 25088) and (512, 25088) in float32, and every row of 6272 rows and fewer; the 112^2 stem tensors in bf16 lose on the
# GPU in both (0.86 - 0.92 x).
ROUTED = {(32, 2, "gelu"): (200704, 802816), (128, 2, "gelu"): (50176, 200704), (512, 2, "gelu"): (12544, 50176),
          (32, 4, "gelu"): (802816, 3211264), (64, 4, "gelu"): (50176, 200704), (128, 4, "gelu"): (200704, 802816)}


def bn_act_routed(n, h, w, c, dtype, epilogue):
    """Whether the routing rule keeps (N, H, W, C) of dtype with this epilogue on the operator: a rule on (R = N H W, C, element size, epilogue) alone."""
    return rows_routed(ROUTED, (int(c), esize(dtype), epilogue), int(n) * int(h) * int(w))


def bn_act_supported(n, h, w, c, dtype, epilogue, measured_only=False, rdtype=None):
    """Whether the kernels take u of (N, H, W, C) and dtype with epilogue "gelu" | "add" (rcx_bn_act_supported: fewer than 2^31 elements; rdtype, the
    dtype of ADD's r, out and g: dtype (the default) or float32) and, with measured_only, the routing rule keeps it (bn_act_routed).  One value a
    channel is refused by the functions, as torch refuses it."""
    rdtype = dtype if rdtype is None else rdtype
    if dtype not in ops._DT or rdtype not in ops._DT or epilogue not in EPILOGUES:
        return False
    if not supported("rcx_bn_act_supported", n, h, w, c, ops._DT[dtype], ops._DT[rdtype], EPILOGUES[epilogue]):
        return False
    return not measured_only or bn_act_routed(n, h, w, c, dtype, epilogue)


def _check_common(fn, u, vecs, epilogue, rdtype=None):
    check_x(fn, u, "u")
    n, c, h, w = u.shape
    for name, t in vecs:
        check_vec(fn, t, c, u.device, name)
    check_rows(n * h * w, tuple(u.shape))
    if not bn_act_supported(n, h, w, c, u.dtype, epilogue, rdtype=rdtype):
        raise ValueError(f"{fn}: no kernel for N={n}, H={h}, W={w}, C={c}, {u.dtype}" + (f" with a {rdtype} residual" if rdtype is not None else "")
                         + " (bn_act_supported)")


def _check_scale(fn, scale, u):
    if scale is not None and (not torch.is_tensor(scale) or scale.dtype != torch.float32 or tuple(scale.shape) != (u.shape[0],) or scale.device != u.device
                              or not scale.is_contiguous()):
        raise ValueError(f"{fn}: scale must be a contiguous float32 ({u.shape[0]},) tensor on {u.device}, or None")


def _forward(epilogue, u, r, scale, weight, bias, running_mean, running_var, momentum, eps):
    n, c, h, w = u.shape
    rdtype = u.dtype if r is None else r.dtype
    out = ops._empty_nhwc(n, c, h, w, rdtype, u.device)
    mean = torch.empty(c, dtype=torch.float32, device=u.device)
    invstd = torch.empty(c, dtype=torch.float32, device=u.device)
    ws, nbytes = workspace("rcx_bn_act_workspace_bytes", u.device, n, h, w, c, ops._DT[u.dtype], ops._DT[rdtype], EPILOGUES[epilogue])
    with ops._on(u.device):
        rc = _lib.load().rcx_bn_act_train_fwd(u.data_ptr(), ptr(r), ptr(scale), out.data_ptr(), weight.data_ptr(), bias.data_ptr(), ptr(running_mean),
                                              ptr(running_var), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), nbytes, n, h, w, c, float(momentum),
                                              float(eps), EPILOGUES[epilogue], ops._dt(u), ops._DT[rdtype], ops._stream(u.device))
    _lib.check(rc, "rcx_bn_act_train_fwd")
    return out, mean, invstd


def _backward(fn, epilogue, u, g, scale, weight, bias, mean, invstd, need_input_grad, need_param_grads):
    if not (need_input_grad or need_param_grads):
        raise ValueError(f"{fn}: no gradient asked for")
    n, c, h, w = u.shape
    gu = ops._empty_nhwc(n, c, h, w, u.dtype, u.device) if need_input_grad else None
    gw = torch.empty(c, dtype=torch.float32, device=u.device) if need_param_grads else None
    gb = torch.empty(c, dtype=torch.float32, device=u.device) if need_param_grads else None
    ws, nbytes = workspace("rcx_bn_act_workspace_bytes", u.device, n, h, w, c, ops._DT[u.dtype], ops._DT[g.dtype], EPILOGUES[epilogue])
    with ops._on(u.device):
        rc = _lib.load().rcx_bn_act_train_bwd(u.data_ptr(), g.data_ptr(), ptr(scale), weight.data_ptr(), ptr(bias), mean.data_ptr(), invstd.data_ptr(),
                                              ptr(gu), ptr(gw), ptr(gb), ws.data_ptr(), nbytes, n, h, w, c, EPILOGUES[epilogue], ops._dt(u),
                                              ops._DT[g.dtype], ops._stream(u.device))
    _lib.check(rc, "rcx_bn_act_train_bwd")
    return gu, gw, gb


def bn_gelu_train(u, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """F.gelu(F.batch_norm(u, running_mean, running_var, weight, bias, training=True, momentum, eps)) on a dense channels_last u of float32 / bfloat16 /
    float16 (rcx_bn_act_train_fwd, RCX_BN_EPI_GELU): -> (z like u, save_mean, save_invstd), the statistics float32 (C) and exactly batch_norm_train's.
    running_mean / running_var (both or neither) are updated in place.  BN(u) is never stored."""
    fn = "bn_gelu_train"
    _check_common(fn, u, (("weight", weight), ("bias", bias)), "gelu")
    check_running(fn, (running_mean, running_var), u.shape[1], u.device, ("running_mean", "running_var"))
    return _forward("gelu", u, None, None, weight, bias, running_mean, running_var, momentum, eps)


def bn_gelu_train_backward(u, gz, weight, bias, mean, invstd, need_input_grad=True, need_param_grads=True):
    """Backward of bn_gelu_train (rcx_bn_act_train_bwd) from u and the forward's saved float32 mean and invstd; gz = dL/dz has u's dtype and layout.
    -> (gu like u | None, gweight float32 (C) | None, gbias float32 (C) | None)."""
    fn = "bn_gelu_train_backward"
    _check_common(fn, u, (("weight", weight), ("bias", bias), ("mean", mean), ("invstd", invstd)), "gelu")
    check_like(fn, gz, "gz", u.shape, (u.dtype,), u.device)
    return _backward(fn, "gelu", u, gz, None, weight, bias, mean, invstd, need_input_grad, need_param_grads)


def bn_add_train(u, r, weight, bias, scale=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5):
    """r + scale.view(N, 1, 1, 1) * F.batch_norm(u, ..., training=True) on dense channels_last u and r (rcx_bn_act_train_fwd, RCX_BN_EPI_ADD): r of u's
    dtype or float32 (an autocast step's residual); scale float32 (N) or None (= 1): the DropPath mask.  -> (out like r, save_mean, save_invstd)."""
    fn = "bn_add_train"
    check_x(fn, u, "u")
    check_like(fn, r, "r", u.shape, (u.dtype, torch.float32), u.device)
    _check_common(fn, u, (("weight", weight), ("bias", bias)), "add", r.dtype)
    check_running(fn, (running_mean, running_var), u.shape[1], u.device, ("running_mean", "running_var"))
    _check_scale(fn, scale, u)
    return _forward("add", u, r, scale, weight, bias, running_mean, running_var, momentum, eps)


def bn_add_train_backward(u, g, weight, mean, invstd, scale=None, need_input_grad=True, need_param_grads=True):
    """Backward of bn_add_train towards u and the norm's parameters (rcx_bn_act_train_bwd): g = dL/dout in out's dtype (u's or float32); the BatchNorm
    backward reads scale[n] g.  dL/dr is g itself and is not computed here.  -> (gu like u | None, gweight | None, gbias | None)."""
    fn = "bn_add_train_backward"
    check_x(fn, u, "u")
    check_like(fn, g, "g", u.shape, (u.dtype, torch.float32), u.device)
    _check_common(fn, u, (("weight", weight), ("mean", mean), ("invstd", invstd)), "add", g.dtype)
    _check_scale(fn, scale, u)
    return _backward(fn, "add", u, g, scale, weight, None, mean, invstd, need_input_grad, need_param_grads)


class BnGeluFn(torch.autograd.Function):
    """GELU(BatchNorm(u)) on batch statistics with a HIP forward and backward: apply(u, weight, bias, running_mean, running_var, momentum, eps) -> z in
    u's dtype.  Saves u, weight, bias, mean and invstd and nothing of u's size besides u; once differentiable; the parameters' gradients come back in
    the parameters' dtype."""

    @staticmethod
    def forward(ctx, u, weight, bias, running_mean, running_var, momentum, eps):
        z, mean, invstd = bn_gelu_train(u, weight.detach(), bias.detach(), running_mean, running_var, momentum, eps)
        ctx.save_for_backward(u, weight, bias, mean, invstd)
        return z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gz):
        u, weight, bias, mean, invstd = ctx.saved_tensors
        need_u, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        if not (need_u or need_p):
            return (None,) * 7
        gu, gw, gb = bn_gelu_train_backward(u, grad_in(gz, u.dtype), weight.detach(), bias.detach(), mean, invstd, need_input_grad=need_u,
                                            need_param_grads=need_p)
        return (gu, *grads_out((gw, gb), (weight.dtype, bias.dtype), ctx.needs_input_grad[1:3]), None, None, None, None)


class BnAddFn(torch.autograd.Function):
    """r + scale[n] BatchNorm(u) on batch statistics with a HIP forward and backward: apply(u, r, scale, weight, bias, running_mean, running_var,
    momentum, eps) -> out in r's dtype (u's or float32).  scale: float32 (N) or None.  Saves u, weight, mean, invstd and scale; once differentiable;
    r's gradient is the incoming gradient itself; the parameters' gradients come back in the parameters' dtype."""

    @staticmethod
    def forward(ctx, u, r, scale, weight, bias, running_mean, running_var, momentum, eps):
        out, mean, invstd = bn_add_train(u, r, weight.detach(), bias.detach(), scale, running_mean, running_var, momentum, eps)
        ctx.save_for_backward(u, weight, mean, invstd, scale)
        ctx.bias_dtype = bias.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        u, weight, mean, invstd, scale = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_u, need_p = need[0], need[3] or need[4]
        gu = gw = gb = None
        if need_u or need_p:
            gd = grad_in(g, g.dtype if g.dtype == torch.float32 else u.dtype)         # float32 (an autocast step's residual) is taken as it is
            gu, gw, gb = bn_add_train_backward(u, gd, weight.detach(), mean, invstd, scale, need_input_grad=need_u, need_param_grads=need_p)
        return (gu, g if need[1] else None, None, *grads_out((gw, gb), (weight.dtype, ctx.bias_dtype), need[3:5]), None, None, None, None)


# ---- what a marked channel mixer / stem runs (models.use_fused_mixer_norms_train) ---------------------------------------------------------------------------

def mark(host, layers, all_shapes):
    """Set the plain attribute on `host` (a channel mixer's nn.Sequential, or a RecNextStem for its ``stem``): the mode and the very layers it was
    marked with.  -> 1 if newly marked."""
    new = 0 if host.__dict__.get(ATTR) else 1
    setattr(host, ATTR, ("all" if all_shapes else "measured",) + tuple(layers))
    return new


def _hooked(*mods):
    """Whether a forward hook or pre-hook is registered on one of the modules themselves."""
    return any(m._forward_hooks or m._forward_pre_hooks for m in mods)


def _conv_norm_ok(cn):
    """A ConvNorm whose norm the operators reproduce (batchnorm.norm_fusable); the replace_batchnorm'ed nn.Conv2d is not one."""
    return isinstance(cn, ConvNorm) and isinstance(cn.conv, nn.Conv2d) and norm_fusable(cn.norm)


def _marked(host, seq, x):
    """The mark's mode if `seq` is still the very layers `host` was marked with and x is a GPU tensor the kernels take, else None."""
    m = host.__dict__.get(ATTR)
    if not m or not gpu_tensor_ok(x):
        return None
    if len(seq) != len(m) - 1 or any(a is not b for a, b in zip(seq, m[1:])):
        return None
    return m[0]


def _routes(u, bn, epilogue, mode, rdtype=None):
    """Whether this norm's call runs on the operator: a 4-D GPU tensor of a dtype and shape the kernels take with more than one value a channel, the
    norm's tensors on its device, and a shape the routing rule keeps (every supported shape in mode "all")."""
    if not (gpu_tensor_ok(u) and u.numel() > u.shape[1]):
        return False
    n, c, h, w = u.shape
    if c != bn.num_features or bn.weight.device != u.device:
        return False
    return bn_act_supported(n, h, w, c, u.dtype, epilogue, measured_only=mode != "all", rdtype=rdtype)


def _bn_gelu(bn, u):
    rm, rv = bump(bn)
    return BnGeluFn.apply(ops._nhwc(u, "u"), bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps)


def mixer_ready(seq, t):
    """The mark's mode if the marked mixer `seq` takes the operators' path for t in this call, else None: still [ConvNorm, exact GELU, ConvNorm] with
    the very layers it was marked with, both norms ones the operators reproduce, a GPU tensor of float32 / bfloat16 / float16, and no forward hook or
    pre-hook on the nn.Sequential, the two ConvNorms or the GELU themselves (a hooked mixer keeps the chain, so that its hooks fire; hooks on the
    convs and the norms fire on either path, except a routed norm's own, whose output is never formed)."""
    mode = _marked(seq, seq, t)
    if mode is None or len(seq) != 3 or not _is_exact_gelu(seq[1]) or not _conv_norm_ok(seq[0]) or not _conv_norm_ok(seq[2]):
        return None
    if _hooked(seq, seq[0], seq[1], seq[2]):               # run_mixer calls .conv and .norm, not these modules: their hooks would not fire
        return None
    return mode


def run_mixer(seq, t, r, drop_path, mode):
    """r + drop_path(seq(t)) of a mixer mixer_ready answered for: seq[0].conv -> BnGeluFn -> seq[2].conv -> BnAddFn, each norm on its operator where
    the routing rule keeps its shape (_routes) and on the module chain -- the very calls nn.Sequential makes -- where not.  The DropPath mask is drawn as
    layers.DropPath.forward draws it, so the random stream and the mask's values are the chain's."""
    u1 = seq[0].conv(t)
    z = _bn_gelu(seq[0].norm, u1) if _routes(u1, seq[0].norm, "gelu", mode) else seq[1](seq[0].norm(u1))
    u2 = seq[2].conv(z)
    bn = seq[2].norm
    plain = drop_path is None or type(drop_path) is nn.Identity
    ok = (plain or type(drop_path) is DropPath) and torch.is_tensor(r) and r.is_cuda and r.shape == u2.shape and r.device == u2.device \
        and r.dtype in (u2.dtype, torch.float32) and _routes(u2, bn, "add", mode, r.dtype)
    if not ok:
        y = bn(u2)
        return r + (y if drop_path is None else drop_path(y))
    scale = None
    if not plain and drop_path.training and drop_path.drop_prob != 0.0:
        keep = 1.0 - drop_path.drop_prob
        scale = u2.new_empty((u2.shape[0], 1, 1, 1)).bernoulli_(keep).div_(keep).float().view(-1)
    rm, rv = bump(bn)
    return BnAddFn.apply(ops._nhwc(u2, "u"), ops._nhwc(r, "r"), scale, bn.weight, bn.bias, rm, rv, bn.momentum, bn.eps)


def stem_ready(stem, x):
    """The mark's mode if the marked RecNextStem takes the operators' path for x in this call, else None: ``stem.stem`` still the very layers, in
    training mode, every ConvNorm's norm one the operators reproduce, no forward hook or pre-hook on ``stem.stem`` or its layers themselves."""
    seq = stem.stem
    mode = _marked(stem, seq, x)
    if mode is None or not stem.training or not all(_conv_norm_ok(m) for m in seq if isinstance(m, ConvNorm)):
        return None
    if _hooked(seq, *seq):                                 # as mixer_ready: a hooked stem keeps the chain
        return None
    return mode


def run_stem(seq, x, mode):
    """seq(x) with every ConvNorm -> exact GELU pair on BnGeluFn where the routing rule keeps its shape; a ConvNorm followed by nn.Identity (or by
    nothing) and every other layer is called as nn.Sequential calls it."""
    i = 0
    while i < len(seq):
        m = seq[i]
        if isinstance(m, ConvNorm) and i + 1 < len(seq) and _is_exact_gelu(seq[i + 1]):
            u = m.conv(x)
            x = _bn_gelu(m.norm, u) if _routes(u, m.norm, "gelu", mode) else seq[i + 1](m.norm(u))
            i += 2
        else:
            x = m(x)
            i += 1
    return x
