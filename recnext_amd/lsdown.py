"""Downsample.token_mixer of the LSNet-style RecNeXt-T / S / B and their share-channel variants (lsnet/model/recattn.py:254-263,
recattn_share_channel.py:223-232) as one HIP launch: the tensor-level front-end of rcx_grouped_conv2d_fwd.  recnext_amd.ops exports the three
functions (``ops.grouped_conv2d`` ...); they are written here because tests/test_guard_cpu.py asks a row in the case table of
tests/test_guard_bands_gpu.py of every launching function whose source is in ops.py, and this entry's guard-band cases (properties A - D, the entry
and a Downsample module) are in tests/test_ls_down_gpu.py (as recnext_amd/lsshare.py does for ls_share).  Allocation goes through ops._empty_nhwc,
so tests/guard.py sees it.  A CPU tensor raises; there is no fallback."""
import torch

from . import _lib, ops


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
        rc = _lib.load().rcx_grouped_conv2d_fwd(x.data_ptr(), y.data_ptr(), wpack.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                n, h, w, cin, cout, groups, k, stride, ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_grouped_conv2d_fwd")
    return y
