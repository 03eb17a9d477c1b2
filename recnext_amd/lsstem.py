"""RecNextStem of the LSNet-style RecNeXt-T / S / B and their share-channel forms (lsnet/model/recattn.py:208-223: three 3x3 stride-2 ConvNorms, a GELU after each
of the first two and, for T and S, after the third) on HIP: the tensor-level front-end of rcx_stem3_fwd (two launches; rcx_stem.hip, rcx_conv3s2.hip).
recnext_amd.ops exports the three functions (``ops.stem3`` ...); they are written here for the reason recnext_amd/lsdown.py gives: the case table of
tests/test_guard_bands_gpu.py lists the launching functions whose source is in ops.py, and this entry's guard-band cases are in tests/test_ls_stem_gpu.py,
which passes this module to tests/guard.py as one of ``modules=`` (the workspace is this module's own ``torch.empty``).  A CPU tensor raises; there is no fallback."""
import torch

from . import _lib, ops


def stem3_supported(n, h, w, c, final_act, dtype):
    """Whether rcx_stem3_fwd has a kernel for the three-conv stem of RecNeXt-T / S / B with C output channels on an N x 3 x H x W input (bf16; C = 64 | 128)."""
    return dtype == torch.bfloat16 and _lib.load().rcx_stem3_supported(int(n), int(h), int(w), int(c), int(bool(final_act)), ops._DT[dtype]) > 0


def pack_stem3(w1, b1, w2, b2, w3, b3):
    """The T / S / B stem's three BN-folded 3x3 stride-2 convs -> (w1p, b1p, w2frag, b2p, w3frag, b3p) for stem3(): w1 (C/4, 3, 3, 3), w2 (C/2, C/4, 3, 3),
    w3 (C, C/2, 3, 3) and their biases.  The first four are pack_stem's; w3frag and b3p are laid out as w2frag and b2p are."""
    c = w3.shape[0]
    if c % 4 or tuple(w1.shape) != (c // 4, 3, 3, 3) or tuple(w2.shape) != (c // 2, c // 4, 3, 3) or tuple(w3.shape) != (c, c // 2, 3, 3):
        raise ValueError(f"stem weights must be (C/4, 3, 3, 3), (C/2, C/4, 3, 3) and (C, C/2, 3, 3), got {tuple(w1.shape)}, {tuple(w2.shape)} and {tuple(w3.shape)}")
    return ops.pack_stem(w1, b1, w2, b2) + ops._pack_conv3x3_frags(w3, b3)


def stem3(x, w1p, b1p, w2frag, b2p, w3frag, b3p, c, final_act):
    """lsmodels.RecNextStem.forward in two launches (rcx_stem3_fwd; lsnet/model/recattn.py:208-223): x N x 3 x H x W channels_last bf16 -> N x C x H3 x W3, the
    planes ceil(/2) three times; final_act: the exact GELU after the third conv (T and S)."""
    if ops._nhwc(x, "x") is not x:                                                # (4-D and on a GPU, or it raises) a copy per forward is not what the caller wants
        raise ValueError(f"x must be channels_last (N x H x W x 3 storage), got shape {tuple(x.shape)} with strides {x.stride()}")
    n, cin, h, w = x.shape
    lib = _lib.load()
    if cin != 3:
        raise ValueError(f"the stem takes 3 input channels, got {cin}")
    if not stem3_supported(n, h, w, c, final_act, x.dtype):
        raise ValueError(f"stem3 has no kernel for C={c} {x.dtype} on {n} x 3 x {h} x {w} (bf16; C = 64 | 128)")
    h3, w3_ = h, w
    for _ in range(3):
        h3, w3_ = -(-h3 // 2), -(-w3_ // 2)
    ops._check_pack(w1p, torch.bfloat16, lib.rcx_stem3_pack_bytes(c, 1) // 2, x.device, "w1p")
    ops._check_pack(b1p, torch.float32, 32, x.device, "b1p")
    ops._check_pack(w2frag, torch.bfloat16, lib.rcx_stem3_pack_bytes(c, 2) // 2, x.device, "w2frag")
    ops._check_pack(b2p, torch.float32, c // 2, x.device, "b2p")
    ops._check_pack(w3frag, torch.bfloat16, lib.rcx_stem3_pack_bytes(c, 3) // 2, x.device, "w3frag")
    ops._check_pack(b3p, torch.float32, c, x.device, "b3p")
    nws = lib.rcx_stem3_workspace_bytes(n, h, w, c)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)                 # the C/2-channel intermediate: written once, read once
    y = ops._empty_nhwc(n, c, h3, w3_, x.dtype, x.device)
    with ops._on(x.device):
        rc = lib.rcx_stem3_fwd(x.data_ptr(), y.data_ptr(), w1p.data_ptr(), b1p.data_ptr(), w2frag.data_ptr(), b2p.data_ptr(), w3frag.data_ptr(), b3p.data_ptr(),
                               ws.data_ptr(), nws, n, h, w, c, int(bool(final_act)), ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_stem3_fwd")
    return y
