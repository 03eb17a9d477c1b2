"""Downsample.token_mixer of the LSNet-style RecNeXt-T / S / B and their share-channel variants (lsnet/model/recattn.py:254-263,
recattn_share_channel.py:223-232) as one HIP launch: the tensor-level front-end of rcx_grouped_conv2d_fwd.  recnext_amd.ops exports the three
functions (``ops.grouped_conv2d`` ...); they are written here because tests/test_guard_cpu.py asks a row in the case table of
tests/test_guard_bands_gpu.py of every launching function whose source is in ops.py, and this entry's guard-band cases (properties A - D, the entry
and a Downsample module) are in tests/test_ls_down_gpu.py (as recnext_amd/lsshare.py does for ls_share).  Allocation goes through ops._empty_nhwc,
so tests/guard.py sees it.  A CPU tensor raises; there is no fallback.

The backward (rcx_grouped_conv2d_bwd: ``grouped_conv2d_backward``, ``unpack_grouped_weight_grad``, ``GroupedConv2dFn``) is here for the same reason; it
allocates its float32 gradients and its workspace with this module's own ``torch.empty``, so its guard-band cases (tests/test_ls_down_bwd_gpu.py) pass
this module to tests/guard.py as one of ``modules=``."""
import torch

from . import _lib, ops
from ._trainop import ptr


def grouped_conv2d_supported(n, h, w, cin, cout, groups, k, stride, dtype):
    """Whether rcx_grouped_conv2d_fwd has a kernel: the grouped 5x5 stride-2 conv with 1 .. 4 channels a group in and out."""
    return dtype in ops._DT and _lib.load().rcx_grouped_conv2d_supported(int(n), int(h), int(w), int(cin), int(cout), int(groups), int(k), int(stride), ops._DT[dtype]) > 0


def pack_grouped_weight(w_oikk):
    """(Cout, Cin / groups, k, k) conv weight -> float32 (k, k, Cin / groups, Cout) on the same device: wpack[((ky k + kx) ci + j) Cout + o] = w[o][j][ky][kx]."""
    if not torch.is_tensor(w_oikk) or w_oikk.dim() != 4 or w_oikk.shape[2] != w_oikk.shape[3]:
        raise ValueError("pack_grouped_weight takes a (Cout, Cin / groups, k, k) weight")
    return w_oikk.detach().float().permute(2, 3, 1, 0).contiguous()


def grouped_conv2d(x, wpack, bias, groups, k=5, stride=2):
    """nn.Conv2d(Cin, Cout, k, stride, padding=k//2, groups=groups) in one launch (rcx_grouped_conv2d_fwd; Downsample.token_mixer of the T / S / B
    families, lsnet/model/recattn.py:254-263): x N x Cin x H x W channels_last -> N x Cout x ceil(H/2) x ceil(W/2) like x.  wpack: pack_grouped_weight's
    float32 (k, k, Cin / groups, Cout); bias float32 (Cout) or None."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError("grouped_conv2d: x must be a 4-D (N, C, H, W) tensor")
    if x.dtype not in ops._DT:
        raise ValueError(f"grouped_conv2d: x must be float32, bfloat16 or float16, got {x.dtype}")
    ops._require_gpu(x, "x")
    n, cin, h, w = x.shape
    groups = int(groups)
    if groups <= 0 or cin % groups:
        raise ValueError(f"grouped_conv2d: groups ({groups}) must divide Cin ({cin})")
    ci = cin // groups
    if not torch.is_tensor(wpack) or wpack.dim() != 4 or tuple(wpack.shape[:3]) != (k, k, ci):
        raise ValueError(f"grouped_conv2d: wpack must be the (k, k, Cin / groups, Cout) = ({k}, {k}, {ci}, Cout) pack of pack_grouped_weight")
    cout = wpack.shape[3]
    ops._check_pack(wpack, torch.float32, k * k * ci * cout, x.device, "wpack")
    if bias is not None:
        ops._check_pack(bias, torch.float32, cout, x.device, "bias")
    if not grouped_conv2d_supported(n, h, w, cin, cout, groups, k, stride, x.dtype):
        raise ValueError(f"grouped_conv2d: no kernel for Cin={cin}, Cout={cout}, groups={groups}, k={k}, stride={stride}, {x.dtype} (grouped_conv2d_supported)")
    x = ops._nhwc(x, "x")
    y = ops._empty_nhwc(n, cout, (h + 1) // 2, (w + 1) // 2, x.dtype, x.device)
    with ops._on(x.device):
        rc = _lib.load().rcx_grouped_conv2d_fwd(x.data_ptr(), y.data_ptr(), wpack.data_ptr(), ptr(bias),
                                                n, h, w, cin, cout, groups, k, stride, ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_grouped_conv2d_fwd")
    return y


def grouped_conv2d_backward_supported(n, h, w, cin, cout, groups, k, stride, dtype):
    """Whether rcx_grouped_conv2d_bwd has kernels: what grouped_conv2d_supported takes."""
    return dtype in ops._DT and _lib.load().rcx_grouped_conv2d_bwd_supported(int(n), int(h), int(w), int(cin), int(cout), int(groups), int(k), int(stride), ops._DT[dtype]) > 0


def grouped_conv2d_backward(x, gy, wpack, groups, need_input_grad=True, need_weight_grad=True, need_bias=False, k=5, stride=2):
    """Backward of grouped_conv2d (rcx_grouped_conv2d_bwd; the training step through Downsample.token_mixer of the T / S / B families,
    lsnet/model/recattn.py:254-263): x N x Cin x H x W and gy N x Cout x ceil(H/2) x ceil(W/2), channels_last, of one dtype; wpack the forward's
    float32 pack.  -> (gx like x | None, gw_pack float32 (k, k, Cin / groups, Cout) | None, gb float32 (Cout) | None).  Deterministic."""
    if not torch.is_tensor(x) or x.dim() != 4 or not torch.is_tensor(gy) or gy.dim() != 4:
        raise ValueError("grouped_conv2d_backward: x and gy must be 4-D (N, C, H, W) tensors")
    if x.dtype not in ops._DT or gy.dtype != x.dtype:
        raise ValueError(f"grouped_conv2d_backward: x and gy must share one of float32, bfloat16 and float16, got {x.dtype} and {gy.dtype}")
    ops._require_gpu(x, "x")
    ops._require_gpu(gy, "gy")
    if not (need_input_grad or need_weight_grad or need_bias):
        raise ValueError("grouped_conv2d_backward: no gradient asked for")
    n, cin, h, w = x.shape
    groups = int(groups)
    if groups <= 0 or cin % groups:
        raise ValueError(f"grouped_conv2d_backward: groups ({groups}) must divide Cin ({cin})")
    ci = cin // groups
    if not torch.is_tensor(wpack) or wpack.dim() != 4 or tuple(wpack.shape[:3]) != (k, k, ci):
        raise ValueError(f"grouped_conv2d_backward: wpack must be the (k, k, Cin / groups, Cout) = ({k}, {k}, {ci}, Cout) pack of pack_grouped_weight")
    cout = wpack.shape[3]
    ops._check_pack(wpack, torch.float32, k * k * ci * cout, x.device, "wpack")
    if tuple(gy.shape) != (n, cout, (h + 1) // 2, (w + 1) // 2) or gy.device != x.device:
        raise ValueError(f"grouped_conv2d_backward: gy has shape {tuple(gy.shape)} on {gy.device}, expected {(n, cout, (h + 1) // 2, (w + 1) // 2)} on {x.device}")
    if not grouped_conv2d_backward_supported(n, h, w, cin, cout, groups, k, stride, x.dtype):
        raise ValueError(f"grouped_conv2d_backward: no kernel for Cin={cin}, Cout={cout}, groups={groups}, k={k}, stride={stride}, {x.dtype} (grouped_conv2d_backward_supported)")
    x = ops._nhwc(x, "x")
    gy = ops._nhwc(gy, "gy")
    lib = _lib.load()
    gx = ops._empty_nhwc(n, cin, h, w, x.dtype, x.device) if need_input_grad else None
    gw = torch.empty((k, k, ci, cout), dtype=torch.float32, device=x.device) if need_weight_grad else None
    gb = torch.empty(cout, dtype=torch.float32, device=x.device) if need_bias else None
    nbytes, ws = 0, None
    if gw is not None or gb is not None:
        nbytes = lib.rcx_grouped_conv2d_bwd_workspace_bytes(n, h, w, cin, cout, groups, k, stride, ops._DT[x.dtype])
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with ops._on(x.device):
        rc = lib.rcx_grouped_conv2d_bwd(x.data_ptr(), gy.data_ptr(), wpack.data_ptr(), ptr(gx), ptr(gw), ptr(gb), ptr(ws), nbytes,
                                        n, h, w, cin, cout, groups, k, stride, ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_grouped_conv2d_bwd")
    return gx, gw, gb


def unpack_grouped_weight_grad(gw_pack):
    """float32 (k, k, Cin / groups, Cout) gradient pack -> (Cout, Cin / groups, k, k), the conv weight's own layout (pack_grouped_weight's inverse)."""
    if not torch.is_tensor(gw_pack) or gw_pack.dim() != 4 or gw_pack.shape[0] != gw_pack.shape[1]:
        raise ValueError("unpack_grouped_weight_grad takes a (k, k, Cin / groups, Cout) pack")
    return gw_pack.permute(3, 2, 0, 1).contiguous()


class GroupedConv2dFn(torch.autograd.Function):
    """nn.Conv2d(Cin, Cout, 5, stride=2, padding=2, groups=groups) with a HIP forward and backward: rcx_grouped_conv2d_fwd / rcx_grouped_conv2d_bwd.
    The output has x's dtype (under autocast: whatever the operator before it produced, as DwConvFn); the parameters' gradients have the parameters'."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups):
        wp = pack_grouped_weight(weight.float())
        bp = bias.detach().float().contiguous() if bias is not None else None
        ctx.save_for_backward(x, wp)
        ctx.groups, ctx.wdtype, ctx.bdtype = int(groups), weight.dtype, (bias.dtype if bias is not None else None)
        return ops.grouped_conv2d(x, wp, bp, groups)

    @staticmethod
    def backward(ctx, gy):
        x, wp = ctx.saved_tensors
        if gy.dtype != x.dtype:
            gy = gy.to(x.dtype)
        gy = gy.contiguous(memory_format=torch.channels_last)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.bdtype is not None and ctx.needs_input_grad[2]
        if not (need_x or need_w or need_b):
            return None, None, None, None
        gx, gw, gb = ops.grouped_conv2d_backward(x, gy, wp, ctx.groups, need_input_grad=need_x, need_weight_grad=need_w, need_bias=need_b)
        return (gx, unpack_grouped_weight_grad(gw).to(ctx.wdtype) if gw is not None else None, gb.to(ctx.bdtype) if gb is not None else None, None)
