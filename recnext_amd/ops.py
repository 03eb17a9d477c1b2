"""Tensor-level front-end of the C ABI: torch supplies device memory and the HIP stream, nothing else.

Every function here requires CUDA(ROCm) tensors and the built HIP library; there is no CPU or
PyTorch-operator fallback (calling with a CPU tensor raises).
"""
import torch

from . import _lib

_DT = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


_D16_CHECKED = set()            # device indices whose D16-hi zero-fill has been verified (rcx_selftest_d16)


def selftest_d16(device):
    """Run the library's start-up probe on `device` (once per process and device; raises RcxError if the hardware does not zero the other half
    of a D16 "hi" load's destination, which the bf16 load paths rely on -- include/recnext_amd.h).  Returns the failure mask (0 = fine)."""
    dev = torch.device(device)
    src = (torch.arange(64, device=dev, dtype=torch.int32) * 517 + 0x1234).to(torch.int16)        # 64 distinct 16-bit patterns
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().rcx_selftest_d16(src.data_ptr(), flag.data_ptr(), _stream(dev))
    _lib.check(rc, "rcx_selftest_d16")
    mask = int(flag.item())
    if mask:
        raise _lib.RcxError(f"D16 self-test failed on {dev} (mask {mask:#x}: bit 0 global_load_short_d16_hi, 1 buffer_load_short_d16_hi, 2 "
                            "ds_read_u16_d16_hi): this device does not zero the other half of a D16-hi load; the 16-bit kernels would return garbage")
    _D16_CHECKED.add(dev.index if dev.index is not None else torch.cuda.current_device())
    return mask


def _dt(t):
    try:
        code = _DT[t.dtype]
    except KeyError:
        raise TypeError(f"recnext_amd kernels take float32, bfloat16 or float16 tensors, got {t.dtype}") from None
    if code != _lib.DTYPE_F32 and t.is_cuda:
        idx = t.device.index
        if idx not in _D16_CHECKED:                      # once per device, before its first 16-bit launch
            if torch.cuda.is_current_stream_capturing():
                # the probe reads its flag back (a synchronisation), which a capturing stream cannot do -- and a captured launch that was never
                # probed would run unguarded on every replay: refuse, loudly, instead of skipping the guard
                raise _lib.RcxError(f"the first 16-bit recnext_amd launch on {t.device} happens while a HIP graph is being captured: call "
                                    "recnext_amd.ops.selftest_d16(device) (or run one eager forward) before the capture")
            selftest_d16(t.device)
            _D16_CHECKED.add(idx)
    return code


def _gy_as_taken(gy, block_dtype, want):
    """dL/dy as a backward entry reads it: as it is when float32, or when it has the block's own dtype and that is the dtype id `want` the
    library's *_bwd_gy_dtype query answered for the problem; converted to float32 otherwise."""
    if gy.dtype == torch.float32 or (gy.dtype == block_dtype and _DT.get(gy.dtype) == want):
        return gy
    return gy.to(torch.float32)


def _require_gpu(t, name):
    if not t.is_cuda:
        raise _lib.RcxError(f"{name} is on {t.device}: the recnext_amd token mixers only run as HIP kernels on a GPU "
                            "(no CPU fallback exists in the product path)")


def _nhwc(t, name="x"):
    """Logical N x C x H x W tensor whose storage is N x H x W x C contiguous (torch.channels_last)."""
    if t.dim() != 4:
        raise ValueError(f"{name} must be 4-D (N,C,H,W), got shape {tuple(t.shape)}")
    _require_gpu(t, name)
    n, c, h, w = t.shape
    want = (h * w * c, 1, w * c, c)
    ok = all(sz == 1 or st == wt for sz, st, wt in zip(t.shape, t.stride(), want))
    if not ok:
        t = t.contiguous(memory_format=torch.channels_last)
        if not all(sz == 1 or st == wt for sz, st, wt in zip(t.shape, t.stride(), want)):
            t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # degenerate-stride corner (C==1 / H==W==1)
    return t


def _empty_nhwc(n, c, h, w, dtype, device):
    return torch.empty((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)


def _empty_flat(numel, dtype, device):
    """A 1-D scratch or gradient block; allocated here, as _empty_nhwc's outputs are, so that tests/guard.py sees what recnext_amd/_trainop.py asks for."""
    return torch.empty(numel, dtype=dtype, device=device)


def _check_bwd_args(fn, x, shapes=(), packs=(), others=()):
    """Extent checks of a backward entry, run before anything is allocated or launched: the C entry points see raw pointers only, so a tensor
    smaller than the extents derived from x would be read out of range on the device.  shapes: (name, tensor, expected shape | None = only x's
    N and C as its first two extents); packs: (name, tensor, element count) of float32 weight packs; others: (name, tensor | None) that must only
    share x's device.  Raises ValueError naming the argument."""
    if x.dim() != 4:
        raise ValueError(f"{fn}: x must be 4-D (N,C,H,W), got shape {tuple(x.shape)}")
    for name, t, want in shapes:
        got = tuple(t.shape)
        if (want is None and (t.dim() != 4 or got[:2] != tuple(x.shape[:2]))) or (want is not None and got != tuple(want)):
            raise ValueError(f"{fn}: {name} has shape {got}, expected " + (f"(N, C) = {tuple(x.shape[:2])} in front of 2-D extents" if want is None else f"{tuple(want)}"))
    for name, t, numel in packs:
        if t.dtype != torch.float32 or t.numel() != numel:
            raise ValueError(f"{fn}: {name} must be a float32 pack of {numel} elements, got {t.numel()} of {t.dtype}")
    for name, t in [(n, t) for n, t, _ in shapes] + [(n, t) for n, t, _ in packs] + list(others):
        if t is not None and t.device != x.device:
            raise ValueError(f"{fn}: {name} is on {t.device}, x on {x.device}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device):
    """The current stream of `device` as a hipStream_t (an integer): the raw getter where this PyTorch has it (0.3 us against 2 us)."""
    if _raw_stream is not None:
        idx = device.index
        return _raw_stream(torch.cuda.current_device() if idx is None else idx)
    return torch.cuda.current_stream(device).cuda_stream


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _on(device):
    """Device guard for a launch: nothing when `device` is already the current device (the usual case; saves ~2 us a call)."""
    idx = device.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(device)


def down_size(h, k):
    p = k // 2
    return (h + 2 * p - k) // 2 + 1


def pack_dw_weight(w, out=None):
    """(C,1,k,k) or (C,k,k) f32/bf16 parameter -> float32 (k,k,C) on the same device."""
    _require_gpu(w, "weight")
    c, k = w.shape[0], w.shape[-1]
    w = w.detach().contiguous()
    if out is None:
        out = torch.empty(k * k * c, dtype=torch.float32, device=w.device)
    with _on(w.device):
        _lib.check(_lib.load().rcx_pack_dw_weight(w.data_ptr(), out.data_ptr(), c, k, _dt(w), _stream(w.device)),
                   "rcx_pack_dw_weight")
    return out


def pack_bias(b, out=None):
    _require_gpu(b, "bias")
    b = b.detach().contiguous()
    if out is None:
        out = torch.empty(b.numel(), dtype=torch.float32, device=b.device)
    with _on(b.device):
        _lib.check(_lib.load().rcx_pack_bias(b.data_ptr(), out.data_ptr(), b.numel(), _dt(b), _stream(b.device)),
                   "rcx_pack_bias")
    return out


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() if t is not None else None for t in tensors])


def pack_recconv_params(w_down, w_convs, b_down=None, b_convs=None, with_flipped=False):
    """-> (wpack (level+2, k*k*C) f32, bpack (level+2, C) f32 | None): [down, convs[0], ..., convs[level]].

    One launch for the whole block (rcx_pack_recconv_params).  with_flipped=True also returns the pack with every k x k
    rotated by 180 degrees -- the taps of the backward's transposed convolutions -- as a third value."""
    ws = [w_down] + list(w_convs)
    c, k = w_down.shape[0], w_down.shape[-1]
    _require_gpu(w_down, "weight")
    for w in ws:
        if tuple(w.shape[-2:]) != (k, k) or w.shape[0] != c:
            raise ValueError("all RecConv2d weights must share (C,1,k,k)")
    dev = w_down.device
    wpack = torch.empty((len(ws), k * k * c), dtype=torch.float32, device=dev)
    bs, bpack = None, None
    if b_down is not None:
        bs = [b_down] + list(b_convs)
        bpack = torch.empty((len(bs), c), dtype=torch.float32, device=dev)
    if any(p.dtype != w_down.dtype or p.device != dev for p in ws + (bs or [])):
        # parameters of mixed dtype: one launch per tensor
        for i, w in enumerate(ws):
            pack_dw_weight(w, wpack[i])
        for i, b in enumerate(bs or []):
            pack_bias(b, bpack[i])
        return (wpack, bpack, wpack.view(len(ws), k, k, c).flip(1, 2).reshape(len(ws), -1).contiguous()) if with_flipped else (wpack, bpack)
    ws = [w.detach().contiguous() for w in ws]
    bs = [b.detach().contiguous() for b in bs] if bs else None
    wflip = torch.empty_like(wpack) if with_flipped else None
    with _on(dev):
        rc = _lib.load().rcx_pack_recconv_params(_ptr_array(ws), _ptr_array(bs) if bs else None, wpack.data_ptr(),
                                                 wflip.data_ptr() if wflip is not None else None,
                                                 bpack.data_ptr() if bpack is not None else None,
                                                 len(ws), c, k, _dt(w_down), _stream(dev))
    _lib.check(rc, "rcx_pack_recconv_params")
    return (wpack, bpack, wflip) if with_flipped else (wpack, bpack)


def unpack_recconv_grads(gwpack, count, c, k):
    """gwpack (count, k*k*C) f32 -> (count, C, 1, k, k) f32, each [i] contiguous in the parameter's layout; one launch."""
    out = torch.empty((count, c, 1, k, k), dtype=torch.float32, device=gwpack.device)
    with _on(gwpack.device):
        rc = _lib.load().rcx_unpack_recconv_grads(gwpack.data_ptr(), _ptr_array([out[i] for i in range(count)]), count, c, k,
                                                  _stream(gwpack.device))
    _lib.check(rc, "rcx_unpack_recconv_grads")
    return out


def reload_options():
    """Re-read the RCX_* environment switches (the library reads them once): for tests and A/B tools that flip one inside a process."""
    _lib.load().rcx_reload_options()


def recconv2d_plan(n, c, h, w, level, k, mode, dtype):
    return _lib.load().rcx_recconv2d_fwd_plan(n, c, h, w, level, k, _lib.MODES[mode], _DT[dtype]).decode()


def recconv2d_bwd_plan(n, c, h, w, level, k, dtype):
    """Which schedule recconv2d_backward would run for these extents and this type (rcx_recconv2d_bwd_plan)."""
    return _lib.load().rcx_recconv2d_bwd_plan(n, c, h, w, level, k, _DT[dtype]).decode()


def recconv2d_bwd_input_plan(n, c, h, w, level, k, dtype):
    """Which schedule recconv2d_input_backward would run for these extents and this type (rcx_recconv2d_bwd_input_plan)."""
    return _lib.load().rcx_recconv2d_bwd_input_plan(n, c, h, w, level, k, _DT[dtype]).decode()


def recconv2d_forward(x, wpack, bpack, level, k, mode="bilinear"):
    """RecConv2d.forward (model/recnext.py:24-34) on the HIP kernels. Returns a channels_last tensor like x."""
    x = _nhwc(x)
    n, c, h, w = x.shape
    if mode not in _lib.MODES:
        raise ValueError(f"mode must be 'bilinear' or 'nearest', got {mode!r}")
    if wpack.numel() != (level + 2) * k * k * c or wpack.dtype != torch.float32:
        raise ValueError("wpack must be float32 of (level+2)*k*k*C elements (see pack_recconv_params)")
    lib = _lib.load()
    dt = _dt(x)
    y = _empty_nhwc(n, c, h, w, x.dtype, x.device)
    nbytes = lib.rcx_recconv2d_fwd_workspace_bytes(n, c, h, w, level, k, dt)    # 0 on the fused schedules: nothing to allocate
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    with _on(x.device):
        rc = lib.rcx_recconv2d_fwd(x.data_ptr(), y.data_ptr(), wpack.data_ptr(),
                                   bpack.data_ptr() if bpack is not None else None,
                                   ws.data_ptr() if ws is not None else None, nbytes, n, c, h, w, level, k, _lib.MODES[mode], dt,
                                   _stream(x.device))
    _lib.check(rc, "rcx_recconv2d_fwd")
    return y


def dwconv2d(x, w_kkc, bias=None, k=5, stride=1, out_dtype=None):
    """Depthwise conv (pad k//2, stride 1|2) with packed float32 (k,k,C) weights."""
    x = _nhwc(x)
    n, c, h, w = x.shape
    out_dtype = out_dtype or x.dtype
    p = k // 2
    ho, wo = (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1
    y = _empty_nhwc(n, c, ho, wo, out_dtype, x.device)
    with _on(x.device):
        rc = _lib.load().rcx_dwconv2d_fwd(x.data_ptr(), y.data_ptr(), w_kkc.data_ptr(),
                                          bias.data_ptr() if bias is not None else None,
                                          n, c, h, w, k, stride, _dt(x), _DT[out_dtype], _stream(x.device))
    _lib.check(rc, "rcx_dwconv2d_fwd")
    return y


def upadd_dwconv_plan(n, c, h, w, hc, wc, k, mode, x_dtype, coarse_dtype=None, out_dtype=None):
    """Which kernel upadd_dwconv would run for these extents and types (rcx_upadd_dwconv_fwd_plan); coarse_dtype None = no coarse plane."""
    return _lib.load().rcx_upadd_dwconv_fwd_plan(n, c, h, w, hc, wc, k, _lib.MODES[mode], _DT[x_dtype],
                                                 _DT[coarse_dtype] if coarse_dtype is not None else _lib.DTYPE_F32,
                                                 _DT[out_dtype or x_dtype], 1 if coarse_dtype is not None else 0).decode()


def upadd_dwconv(x, coarse, w_kkc, bias=None, k=5, mode="nearest", out_dtype=None):
    """dwconv_k(x + resize(coarse -> size(x), mode)); coarse may be None."""
    x = _nhwc(x)
    n, c, h, w = x.shape
    out_dtype = out_dtype or x.dtype
    hc = wc = 0
    cdt = _lib.DTYPE_F32
    if coarse is not None:
        coarse = _nhwc(coarse, "coarse")
        if coarse.shape[0] != n or coarse.shape[1] != c:
            raise ValueError("coarse must share N and C with x")
        hc, wc = coarse.shape[2:]
        cdt = _dt(coarse)
    y = _empty_nhwc(n, c, h, w, out_dtype, x.device)
    with _on(x.device):
        rc = _lib.load().rcx_upadd_dwconv_fwd(x.data_ptr(), coarse.data_ptr() if coarse is not None else None, y.data_ptr(),
                                              w_kkc.data_ptr(), bias.data_ptr() if bias is not None else None,
                                              n, c, h, w, hc, wc, k, _lib.MODES[mode], _dt(x), cdt, _DT[out_dtype],
                                              _stream(x.device))
    _lib.check(rc, "rcx_upadd_dwconv_fwd")
    return y


def dwconv2d_mult2(x, w_kkc, bias=None, k=7, stride=2):
    """nn.Conv2d(C, 2C, k, stride, padding=k//2, groups=C) with packed float32 (k,k,2C) weights."""
    x = _nhwc(x)
    n, c, h, w = x.shape
    p = k // 2
    ho, wo = (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1
    y = _empty_nhwc(n, 2 * c, ho, wo, x.dtype, x.device)
    with _on(x.device):
        rc = _lib.load().rcx_dwconv2d_mult2_fwd(x.data_ptr(), y.data_ptr(), w_kkc.data_ptr(),
                                                bias.data_ptr() if bias is not None else None,
                                                n, c, h, w, k, stride, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_dwconv2d_mult2_fwd")
    return y


def _conv_out_shape(x, mult, k, stride):
    n, c, h, w = x.shape
    p = k // 2
    return (n, c * mult, (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1)


def dwconv2d_backward(x, gy, w_kkc, k, stride, need_input_grad=True, need_bias=False):
    """Backward of dwconv2d: -> (gx like x | None, gw (k,k,C) float32, gb (C) float32 | None). Deterministic."""
    _check_bwd_args("dwconv2d_backward", x, shapes=[("gy", gy, _conv_out_shape(x, 1, k, stride))], packs=[("w_kkc", w_kkc, k * k * x.shape[1])])
    x = _nhwc(x)
    n, c, h, w = x.shape
    gy = _nhwc(gy.to(torch.float32), "grad_output")
    lib = _lib.load()
    wflip = w_kkc.view(k, k, c).flip(0, 1).contiguous()
    gx = _empty_nhwc(n, c, h, w, x.dtype, x.device) if need_input_grad else None
    gw = torch.empty(k * k * c, dtype=torch.float32, device=x.device)
    gb = torch.empty(c, dtype=torch.float32, device=x.device) if need_bias else None
    nbytes = lib.rcx_dwconv2d_bwd_workspace_bytes(c, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    with _on(x.device):
        rc = lib.rcx_dwconv2d_bwd(x.data_ptr(), gy.data_ptr(), w_kkc.data_ptr(), wflip.data_ptr(),
                                  gx.data_ptr() if gx is not None else None, gw.data_ptr(), gb.data_ptr() if gb is not None else None,
                                  ws.data_ptr(), nbytes, n, c, h, w, k, stride, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_dwconv2d_bwd")
    return gx, gw, gb


def upadd_dwconv_backward(x, coarse, gy, w_kkc, k=5, mode="nearest", need_input_grad=True, need_coarse_grad=True, need_bias=False):
    """Backward of upadd_dwconv with a coarse plane (rcx_upadd_dwconv_bwd; model/recattn.py:67): -> (gx like x | None, gcoarse float32 like coarse | None,
    gw (k,k,C) float32, gb (C) float32 | None).  coarse must be float32; gy float32 or (where the library takes it) x's own 16-bit dtype.  Deterministic."""
    _check_bwd_args("upadd_dwconv_backward", x, shapes=[("coarse", coarse, None), ("gy", gy, x.shape)], packs=[("w_kkc", w_kkc, k * k * x.shape[1])])
    x = _nhwc(x)
    coarse = _nhwc(coarse, "coarse")
    if coarse.dtype != torch.float32:
        raise TypeError("upadd_dwconv_backward takes the coarse plane in float32")
    n, c, h, w = x.shape
    hc, wc = coarse.shape[2:]
    lib = _lib.load()
    want = lib.rcx_upadd_dwconv_bwd_gy_dtype(n, c, h, w, hc, wc, k, _dt(x))
    gy = _nhwc(_gy_as_taken(gy, x.dtype, want), "grad_output")
    wflip = w_kkc.view(k, k, c).flip(0, 1).contiguous()
    gx = _empty_nhwc(n, c, h, w, x.dtype, x.device) if need_input_grad else None
    gc = _empty_nhwc(n, c, hc, wc, torch.float32, x.device) if need_coarse_grad else None
    gw = torch.empty(k * k * c, dtype=torch.float32, device=x.device)
    gb = torch.empty(c, dtype=torch.float32, device=x.device) if need_bias else None
    nbytes = lib.rcx_upadd_dwconv_bwd_workspace_bytes(n, c, h, w, hc, wc, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    with _on(x.device):
        rc = lib.rcx_upadd_dwconv_bwd(x.data_ptr(), coarse.data_ptr(), gy.data_ptr(), _DT[gy.dtype], w_kkc.data_ptr(), wflip.data_ptr(),
                                      gx.data_ptr() if gx is not None else None, gc.data_ptr() if gc is not None else None, gw.data_ptr(),
                                      gb.data_ptr() if gb is not None else None, ws.data_ptr(), nbytes, n, c, h, w, hc, wc, k, _lib.MODES[mode], _dt(x),
                                      _stream(x.device))
    _lib.check(rc, "rcx_upadd_dwconv_bwd")
    return gx, gc, gw, gb


def dwconv2d_mult2_backward(x, gy, w_kkc, k, need_input_grad=True, need_bias=False):
    """Backward of dwconv2d_mult2 (stride 2): -> (gx like x | None, gw (k,k,2C) float32, gb (2C) float32 | None)."""
    _check_bwd_args("dwconv2d_mult2_backward", x, shapes=[("gy", gy, _conv_out_shape(x, 2, k, 2))], packs=[("w_kkc", w_kkc, k * k * 2 * x.shape[1])])
    x = _nhwc(x)
    n, c, h, w = x.shape
    gy = _nhwc(gy.to(torch.float32), "grad_output")
    lib = _lib.load()
    gx = _empty_nhwc(n, c, h, w, x.dtype, x.device) if need_input_grad else None
    gw = torch.empty(k * k * 2 * c, dtype=torch.float32, device=x.device)
    gb = torch.empty(2 * c, dtype=torch.float32, device=x.device) if need_bias else None
    nbytes = lib.rcx_dwconv2d_bwd_workspace_bytes(2 * c, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    with _on(x.device):
        rc = lib.rcx_dwconv2d_mult2_bwd(x.data_ptr(), gy.data_ptr(), w_kkc.data_ptr(), gx.data_ptr() if gx is not None else None,
                                        gw.data_ptr(), gb.data_ptr() if gb is not None else None, ws.data_ptr(), nbytes,
                                        n, c, h, w, k, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_dwconv2d_mult2_bwd")
    return gx, gw, gb


def linear_attention_core(qpre, kpre, v, pe, heads):
    """Everything after the qk projection of LinearAttention1/2 (model/recattn.py:21-28, :44-51).

    qpre, kpre: (B, n, C) pre-activations; v, pe: N x C x h x w channels_last (viewed as (B, n, C)); returns channels_last like v.
    """
    v = _nhwc(v, "v")
    pe = _nhwc(pe, "pe")
    b, c, h, w = v.shape
    n = h * w
    for t, name in ((qpre, "qpre"), (kpre, "kpre")):
        _require_gpu(t, name)
        if tuple(t.shape) != (b, n, c) or not t.is_contiguous() or t.dtype != v.dtype:
            raise ValueError(f"{name} must be a contiguous ({b}, {n}, {c}) tensor of {v.dtype}, got {tuple(t.shape)} {t.dtype}")
    if pe.shape != v.shape or pe.dtype != v.dtype:
        raise ValueError("pe must match v")
    out = _empty_nhwc(b, c, h, w, v.dtype, v.device)
    with _on(v.device):
        rc = _lib.load().rcx_linear_attention_fwd(qpre.data_ptr(), kpre.data_ptr(), v.data_ptr(), pe.data_ptr(), out.data_ptr(),
                                                  b, n, c, heads, _dt(v), _stream(v.device))
    _lib.check(rc, "rcx_linear_attention_fwd")
    return out


def linear_attention_core_fuses_pe(c, heads):
    """Whether linear_attention_core_pe has a kernel for this head size (a multiple of four, at most 64)."""
    d = c // heads
    return c % heads == 0 and d % 4 == 0 and d <= 64


def linear_attention_core_pe(qpre, kpre, v, w_pe_kkc, b_pe, heads):
    """linear_attention_core with pe = dwconv3x3(v) + bias computed inside the kernel (rcx_linear_attention_pe_fwd): w_pe_kkc / b_pe are
    the float32 packs of pack_dw_weight / pack_bias of LinearAttention.pe (BatchNorm folded).  None if the library has no such kernel for
    this configuration (the long sequences that run on the matrix cores: measured slower there)."""
    v = _nhwc(v, "v")
    b, c, h, w = v.shape
    n = h * w
    for t, name in ((qpre, "qpre"), (kpre, "kpre")):
        _require_gpu(t, name)
        if tuple(t.shape) != (b, n, c) or not t.is_contiguous() or t.dtype != v.dtype:
            raise ValueError(f"{name} must be a contiguous ({b}, {n}, {c}) tensor of {v.dtype}, got {tuple(t.shape)} {t.dtype}")
    if w_pe_kkc.dtype != torch.float32 or w_pe_kkc.numel() != 9 * c:
        raise ValueError("w_pe_kkc must be the float32 (3, 3, C) pack of pack_dw_weight")
    out = _empty_nhwc(b, c, h, w, v.dtype, v.device)
    with _on(v.device):
        rc = _lib.load().rcx_linear_attention_pe_fwd(qpre.data_ptr(), kpre.data_ptr(), v.data_ptr(), w_pe_kkc.data_ptr(),
                                                     b_pe.data_ptr() if b_pe is not None else None, out.data_ptr(),
                                                     b, h, w, c, heads, _dt(v), _stream(v.device))
    if rc == _lib.ERR_UNSUPPORTED:       # the matrix-core kernel has no such form: the caller runs the two steps
        return None
    _lib.check(rc, "rcx_linear_attention_pe_fwd")
    return out


def recattn_qkcore_supported(c, heads, h, w):
    """Whether recattn_qkcore has a kernel for this coarse plane (rcx_recattn_qkcore_launches: 1/2/4/8/16 heads of 32 channels, or of 4 .. 28 in fours when heads is even, or 2/4/8
    heads of 36 .. 64 in fours (RecNeXt-A5's 40); one launch for planes of at most 64 tokens that fit the LDS, two launches otherwise)."""
    return _lib.load().rcx_recattn_qkcore_launches(1, h, w, c, heads) > 0


def recattn_qkcore(d, wqk_bf16, bqk, w_pe_kkc, b_pe, heads):
    """RecAttn2d's coarse level on the matrix cores (rcx_recattn_qkcore_fwd; one launch up to 64 tokens, two above): d float32 N x C x h x w channels_last; wqk_bf16 (2C, C/2) bfloat16, bqk (2C)
    float32, the pe packs as linear_attention_core_pe.  Returns the attention output + pe, float32 channels_last like d."""
    d = _nhwc(d, "d")
    b, c, h, w = d.shape
    if d.dtype != torch.float32:
        raise ValueError("d must be float32 (the coarse chain of RecAttn2d)")
    if wqk_bf16.dtype != torch.bfloat16 or tuple(wqk_bf16.shape) != (2 * c, c // 2) or not wqk_bf16.is_contiguous():
        raise ValueError(f"wqk_bf16 must be a contiguous ({2 * c}, {c // 2}) bfloat16 tensor")
    if bqk.dtype != torch.float32 or bqk.numel() != 2 * c:
        raise ValueError("bqk must be float32 of 2C elements")
    out = _empty_nhwc(b, c, h, w, torch.float32, d.device)
    lib = _lib.load()
    need = lib.rcx_recattn_qkcore_workspace_bytes(b, h, w, c, heads)               # the k^T v partial sums of the two-launch form (> 64 tokens)
    ws = torch.empty(need, dtype=torch.uint8, device=d.device) if need else None
    with _on(d.device):
        rc = lib.rcx_recattn_qkcore_fwd(d.data_ptr(), wqk_bf16.data_ptr(), bqk.data_ptr(), w_pe_kkc.data_ptr(),
                                        b_pe.data_ptr() if b_pe is not None else None, out.data_ptr(),
                                        ws.data_ptr() if ws is not None else None, need, b, h, w, c, heads, _stream(d.device))
    _lib.check(rc, "rcx_recattn_qkcore_fwd")
    return out


def recattn_down_qkcore_supported(c, heads, h, w, x_dtype):
    """Whether RecAttn2d's stride-2 conv + coarse level run as ONE launch from x (rcx_recattn_down_qkcore_fwd: the 14 x 14 and 7 x 7 planes of 16-bit
    activations; heads as recattn_qkcore_supported, where the coarse plane's image fits the LDS)."""
    return x_dtype in _DT and _lib.load().rcx_recattn_down_qkcore_supported(1, h, w, c, heads, _DT[x_dtype]) > 0


def recattn_down_qkcore(x, w_down_kkc, b_down, wqk_bf16, bqk, w_pe_kkc, b_pe, heads):
    """a = LinearAttention(ConvNorm_k5s2(x)) of RecAttn2d.forward (model/recattn.py:61-66) in one launch: x N x C x H x W channels_last, 16-bit; the conv's
    packs as dwconv2d takes them, the rest as recattn_qkcore.  Returns float32 N x C x ceil(H/2) x ceil(W/2), channels_last."""
    x = _nhwc(x, "x")
    b, c, h, w = x.shape
    if wqk_bf16.dtype != torch.bfloat16 or tuple(wqk_bf16.shape) != (2 * c, c // 2) or not wqk_bf16.is_contiguous():
        raise ValueError(f"wqk_bf16 must be a contiguous ({2 * c}, {c // 2}) bfloat16 tensor")
    if bqk.dtype != torch.float32 or bqk.numel() != 2 * c:
        raise ValueError("bqk must be float32 of 2C elements")
    out = _empty_nhwc(b, c, (h + 1) // 2, (w + 1) // 2, torch.float32, x.device)
    with _on(x.device):
        rc = _lib.load().rcx_recattn_down_qkcore_fwd(x.data_ptr(), w_down_kkc.data_ptr(), b_down.data_ptr() if b_down is not None else None,
                                                     wqk_bf16.data_ptr(), bqk.data_ptr(), w_pe_kkc.data_ptr(),
                                                     b_pe.data_ptr() if b_pe is not None else None, out.data_ptr(), b, h, w, c, heads, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_recattn_down_qkcore_fwd")
    return out


def recattn2d_supported(c, heads, h, w, mode, dtype):
    """Whether RecAttn2d.forward is ONE launch for this plane (rcx_recattn2d_fwd: 14 x 14 / 7 x 7, 1 .. 8 heads of 32 (or 4 .. 28; never wider), nearest, 16-bit)."""
    return dtype in _DT and mode in _lib.MODES and _lib.load().rcx_recattn2d_fwd_supported(1, h, w, c, heads, _lib.MODES[mode], _DT[dtype]) > 0


def recattn2d(x, w_down_kkc, b_down, wqk_bf16, bqk, w_pe_kkc, b_pe, w_conv_kkc, b_conv, heads, mode="nearest"):
    """RecAttn2d.forward (eval, BatchNorms folded; model/recattn.py:54-67) in one launch: x N x C x H x W channels_last, 16-bit -> y like x."""
    x = _nhwc(x, "x")
    b, c, h, w = x.shape
    if wqk_bf16.dtype != torch.bfloat16 or tuple(wqk_bf16.shape) != (2 * c, c // 2) or not wqk_bf16.is_contiguous():
        raise ValueError(f"wqk_bf16 must be a contiguous ({2 * c}, {c // 2}) bfloat16 tensor")
    if bqk.dtype != torch.float32 or bqk.numel() != 2 * c:
        raise ValueError("bqk must be float32 of 2C elements")
    y = torch.empty_like(x, memory_format=torch.channels_last)
    p = lambda t: t.data_ptr() if t is not None else None
    with _on(x.device):
        rc = _lib.load().rcx_recattn2d_fwd(x.data_ptr(), y.data_ptr(), w_down_kkc.data_ptr(), p(b_down), wqk_bf16.data_ptr(), bqk.data_ptr(),
                                           w_pe_kkc.data_ptr(), p(b_pe), w_conv_kkc.data_ptr(), p(b_conv), b, h, w, c, heads, _lib.MODES[mode], _dt(x),
                                           _stream(x.device))
    _lib.check(rc, "rcx_recattn2d_fwd")
    return y


def ls_recattn_supported(b, h, w, c, split, heads, dtype):
    """Whether rcx_ls_recattn_fwd has a kernel for the token half of an LSNet-style RecNeXt block whose slice mixer is RecAttn2d (one head of `split` channels)."""
    return dtype in _DT and _lib.load().rcx_ls_recattn_supported(b, h, w, c, split, heads, _DT[dtype]) > 0


def ls_la3_supported(b, h, w, c, split, heads, dtype):
    """Whether rcx_ls_la3_fwd has a kernel for the token half whose slice mixer is LinearAttention3 (`heads` = the module's own num_heads)."""
    return dtype in _DT and _lib.load().rcx_ls_la3_supported(b, h, w, c, split, heads, _DT[dtype]) > 0


def _check_ls_args(fn, x, split, packs):
    """Shape / dtype / device checks of a token-half entry, before anything is allocated or launched.  packs: (name, tensor, element count)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"{fn}: x must be a 4-D (N, C, H, W) tensor")
    if x.dtype not in _DT:
        raise ValueError(f"{fn}: x must be float32, bfloat16 or float16, got {x.dtype}")
    _require_gpu(x, "x")
    c = x.shape[1]
    if not (0 < split <= c) or split % 4 or c % 4:
        raise ValueError(f"{fn}: C ({c}) and split ({split}) must be multiples of 4 with 0 < split <= C")
    for name, t, numel in packs:
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != numel or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be a contiguous float32 tensor of {numel} elements")
        if t.device != x.device:
            raise ValueError(f"{fn}: {name} is on {t.device}, x on {x.device}")


def ls_recattn(x, w_rep, b_rep, w_down_kkc, b_down, wqT, bq, wkT, bk, w_pe_kkc, b_pe, w_conv_kkc, b_conv, split, heads=1):
    """The token half of an LSNet-style RecNeXt block whose slice mixer is RecAttn2d (lsnet/model/recattn.py:8-34, :115-127, :226-251; eval, BatchNorms folded):
    x (N, C, H, W) channels_last -> (r, t), r = RepVGGDW(x), t = cat(RecAttn2d(r[:, :split]), r[:, split:]), both like x.  Packs: w_rep / b_rep the folded
    RepVGGDW ((3,3,C) / C), the slice's convs as (k,k,split) / split packs, wqT / wkT (split/2, split) the transposed q / k rows of the folded grouped `qk`."""
    c = x.shape[1] if torch.is_tensor(x) and x.dim() == 4 else 0
    _check_ls_args("ls_recattn", x, split, [("w_rep", w_rep, 9 * c), ("b_rep", b_rep, c), ("w_down_kkc", w_down_kkc, 25 * split), ("b_down", b_down, split),
                                            ("wqT", wqT, split * (split // 2)), ("bq", bq, split), ("wkT", wkT, split * (split // 2)), ("bk", bk, split),
                                            ("w_pe_kkc", w_pe_kkc, 9 * split), ("b_pe", b_pe, split), ("w_conv_kkc", w_conv_kkc, 25 * split), ("b_conv", b_conv, split)])
    b, _, h, w = x.shape
    if not ls_recattn_supported(b, h, w, c, split, heads, x.dtype):
        raise ValueError(f"ls_recattn: no kernel for a {h} x {w} plane, C={c}, split={split}, {heads} heads, {x.dtype} (ls_recattn_supported)")
    x = _nhwc(x, "x")
    r = torch.empty_like(x, memory_format=torch.channels_last)
    t = torch.empty_like(x, memory_format=torch.channels_last)
    with _on(x.device):
        rc = _lib.load().rcx_ls_recattn_fwd(x.data_ptr(), r.data_ptr(), t.data_ptr(), w_rep.data_ptr(), b_rep.data_ptr(), w_down_kkc.data_ptr(), b_down.data_ptr(),
                                            wqT.data_ptr(), bq.data_ptr(), wkT.data_ptr(), bk.data_ptr(), w_pe_kkc.data_ptr(), b_pe.data_ptr(),
                                            w_conv_kkc.data_ptr(), b_conv.data_ptr(), b, h, w, c, split, heads, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_ls_recattn_fwd")
    return r, t


def ls_la3(x, w_rep, b_rep, wqT, bq, wkT, bk, w_pe_kkc, b_pe, split, heads):
    """The token half whose slice mixer is LinearAttention3 (lsnet/model/recattn.py:89-112; `heads` = the module's own num_heads): x -> (r, t) as ls_recattn.
    wqT / wkT (split, split/2): the transposed q rows [0, split/2) and k rows [split/2, split) of the folded full 1x1 `qk`."""
    c = x.shape[1] if torch.is_tensor(x) and x.dim() == 4 else 0
    _check_ls_args("ls_la3", x, split, [("w_rep", w_rep, 9 * c), ("b_rep", b_rep, c), ("wqT", wqT, split * (split // 2)), ("bq", bq, split // 2),
                                        ("wkT", wkT, split * (split // 2)), ("bk", bk, split // 2), ("w_pe_kkc", w_pe_kkc, 9 * split), ("b_pe", b_pe, split)])
    b, _, h, w = x.shape
    if not ls_la3_supported(b, h, w, c, split, heads, x.dtype):
        raise ValueError(f"ls_la3: no kernel for a {h} x {w} plane, C={c}, split={split}, {heads} heads, {x.dtype} (ls_la3_supported)")
    x = _nhwc(x, "x")
    r = torch.empty_like(x, memory_format=torch.channels_last)
    t = torch.empty_like(x, memory_format=torch.channels_last)
    with _on(x.device):
        rc = _lib.load().rcx_ls_la3_fwd(x.data_ptr(), r.data_ptr(), t.data_ptr(), w_rep.data_ptr(), b_rep.data_ptr(), wqT.data_ptr(), bq.data_ptr(),
                                        wkT.data_ptr(), bk.data_ptr(), w_pe_kkc.data_ptr(), b_pe.data_ptr(), b, h, w, c, split, heads, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_ls_la3_fwd")
    return r, t


def ls_recattn_tiled_supported(b, h, w, c, split, heads, dtype):
    """Whether rcx_ls_recattn_tiled_fwd (ls_recattn's function on any plane size, the image cut into token chunks) has a kernel for the shape."""
    return dtype in _DT and _lib.load().rcx_ls_recattn_tiled_supported(b, h, w, c, split, heads, _DT[dtype]) > 0


def ls_la3_tiled_supported(b, h, w, c, split, heads, dtype):
    """Whether rcx_ls_la3_tiled_fwd (ls_la3's function on any plane size) has a kernel for the shape."""
    return dtype in _DT and _lib.load().rcx_ls_la3_tiled_supported(b, h, w, c, split, heads, _DT[dtype]) > 0


def _ls_workspace(x, nbytes, workspace):
    """The float32 workspace of a tiled token half: the caller's (checked) or one from torch's allocator on the current stream."""
    if workspace is None:
        return torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    if not torch.is_tensor(workspace) or workspace.dtype != torch.float32 or workspace.device != x.device or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous float32 tensor on x's device")
    if workspace.numel() * 4 < nbytes:
        raise ValueError(f"workspace of {workspace.numel() * 4} bytes, {nbytes} needed")
    return workspace


def ls_recattn_tiled(x, w_rep, b_rep, w_down_kkc, b_down, wqT, bq, wkT, bk, w_pe_kkc, b_pe, w_conv_kkc, b_conv, split, heads=1, workspace=None):
    """ls_recattn's function and arguments for any H x W (rcx_ls_recattn_tiled_fwd: four launches, the image-wide sums through a float32 workspace
    from torch's allocator unless `workspace` is given).  Deterministic; a batch and its shards give the same rows bit for bit."""
    c = x.shape[1] if torch.is_tensor(x) and x.dim() == 4 else 0
    _check_ls_args("ls_recattn_tiled", x, split, [("w_rep", w_rep, 9 * c), ("b_rep", b_rep, c), ("w_down_kkc", w_down_kkc, 25 * split), ("b_down", b_down, split),
                                                  ("wqT", wqT, split * (split // 2)), ("bq", bq, split), ("wkT", wkT, split * (split // 2)), ("bk", bk, split),
                                                  ("w_pe_kkc", w_pe_kkc, 9 * split), ("b_pe", b_pe, split), ("w_conv_kkc", w_conv_kkc, 25 * split), ("b_conv", b_conv, split)])
    b, _, h, w = x.shape
    if not ls_recattn_tiled_supported(b, h, w, c, split, heads, x.dtype):
        raise ValueError(f"ls_recattn_tiled: no kernel for a {h} x {w} plane, C={c}, split={split}, {heads} heads, {x.dtype} (ls_recattn_tiled_supported)")
    lib = _lib.load()
    nbytes = lib.rcx_ls_recattn_tiled_workspace_bytes(b, h, w, c, split, heads, _dt(x))
    x = _nhwc(x, "x")
    with _on(x.device):
        ws = _ls_workspace(x, nbytes, workspace)
        r = torch.empty_like(x, memory_format=torch.channels_last)
        t = torch.empty_like(x, memory_format=torch.channels_last)
        rc = lib.rcx_ls_recattn_tiled_fwd(x.data_ptr(), r.data_ptr(), t.data_ptr(), w_rep.data_ptr(), b_rep.data_ptr(), w_down_kkc.data_ptr(), b_down.data_ptr(),
                                          wqT.data_ptr(), bq.data_ptr(), wkT.data_ptr(), bk.data_ptr(), w_pe_kkc.data_ptr(), b_pe.data_ptr(),
                                          w_conv_kkc.data_ptr(), b_conv.data_ptr(), ws.data_ptr(), ws.numel() * 4, b, h, w, c, split, heads, _dt(x),
                                          _stream(x.device))
    _lib.check(rc, "rcx_ls_recattn_tiled_fwd")
    return r, t


def ls_la3_tiled(x, w_rep, b_rep, wqT, bq, wkT, bk, w_pe_kkc, b_pe, split, heads, workspace=None):
    """ls_la3's function and arguments for any H x W (rcx_ls_la3_tiled_fwd: three launches; the workspace as ls_recattn_tiled)."""
    c = x.shape[1] if torch.is_tensor(x) and x.dim() == 4 else 0
    _check_ls_args("ls_la3_tiled", x, split, [("w_rep", w_rep, 9 * c), ("b_rep", b_rep, c), ("wqT", wqT, split * (split // 2)), ("bq", bq, split // 2),
                                              ("wkT", wkT, split * (split // 2)), ("bk", bk, split // 2), ("w_pe_kkc", w_pe_kkc, 9 * split), ("b_pe", b_pe, split)])
    b, _, h, w = x.shape
    if not ls_la3_tiled_supported(b, h, w, c, split, heads, x.dtype):
        raise ValueError(f"ls_la3_tiled: no kernel for a {h} x {w} plane, C={c}, split={split}, {heads} heads, {x.dtype} (ls_la3_tiled_supported)")
    lib = _lib.load()
    nbytes = lib.rcx_ls_la3_tiled_workspace_bytes(b, h, w, c, split, heads, _dt(x))
    x = _nhwc(x, "x")
    with _on(x.device):
        ws = _ls_workspace(x, nbytes, workspace)
        r = torch.empty_like(x, memory_format=torch.channels_last)
        t = torch.empty_like(x, memory_format=torch.channels_last)
        rc = lib.rcx_ls_la3_tiled_fwd(x.data_ptr(), r.data_ptr(), t.data_ptr(), w_rep.data_ptr(), b_rep.data_ptr(), wqT.data_ptr(), bq.data_ptr(),
                                      wkT.data_ptr(), bk.data_ptr(), w_pe_kkc.data_ptr(), b_pe.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                      b, h, w, c, split, heads, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_ls_la3_tiled_fwd")
    return r, t


def _mlp_acc_unit(i, h):
    """Hidden unit (within a 32-unit tile) that accumulator register i of lane half h holds after the first product (rcx_mlp.hip acc_row)."""
    return (i & 3) + 8 * (i >> 2) + 4 * h


def channel_mlp_hidden(m, c, hidden, dtype):
    """The hidden width rcx_channel_mlp_fwd would run M tokens of C channels and `hidden` units at (the next multiple of 32, 64 or 128 it has a kernel
    for: zero units change nothing), or 0 when it has none (bf16 only)."""
    if dtype != torch.bfloat16:
        return 0
    lib = _lib.load()
    for mult in (32, 64, 128):
        hp = -(-int(hidden) // mult) * mult
        if hp <= 1.125 * hidden + 31 and lib.rcx_channel_mlp_supported(int(m), int(c), hp, _DT[dtype]) > 0:
            return hp
    return 0


def channel_mlp_supported(m, c, hidden, dtype):
    return channel_mlp_hidden(m, c, hidden, dtype) > 0


def _mlp_tiles(c, hidden):
    """(KS1, HT, CT) of a channel mixer of C channels and `hidden` (a multiple of 32) units: k-steps of the first product, hidden tiles, output tiles -- the
    rule of rcx_mlp.hip's mlp_ks1 / mlp_ct (tests/test_mlp768_cpu.py holds the two together through rcx_channel_mlp_pack_bytes)."""
    ks1, ht, ct = -(-c // 16), hidden // 32, -(-c // 32)
    if c > 128 and ct % 2:                  # the streamed kernels write y in halves of two output tiles: one more tile of zero rows
        ct += 1
    return ks1, ht, ct


def pack_channel_mlp(w1, b1, w2, b2, hidden_to=None):
    """The two BN-folded 1x1 convs of a channel mixer -> (wfrag, bias, H) for channel_mlp: w1 (H0, C[, 1, 1]), b1 (H0) | None, w2 (C, H0[, 1, 1]), b2 (C) | None;
    hidden_to: the padded hidden width H (channel_mlp_hidden; default the next multiple of 32).

    The hidden layer is padded with zero units to H = a multiple of 32, C to whole k-steps / output tiles with zero columns / rows; the weights are rounded to
    bf16 (they already are bf16 in a bf16 model) and laid out fragment by fragment in the order the kernel's lanes read them (rcx_mlp.hip):
      W1 fragment (ht, ks), lane (h, m), element j = W1[32 ht + m][16 ks + 8 h + j]
      W2 fragment (ht, ct, q), lane (h, m), element j = 0.5 W2[32 ct + m][32 ht + unit(8 q + j, h)]      unit = _mlp_acc_unit: the order the first product leaves in the registers
    stored hidden tile by hidden tile: [W1 (ht, 0 .. KS1-1)] [W2 (ht, ct, q) for ct, q] for ht = 0 .. H/32 - 1, 1 KB (64 lanes x 8 bf16) per fragment.
    """
    w1 = w1.detach().reshape(w1.shape[0], -1)
    w2 = w2.detach().reshape(w2.shape[0], -1)
    h0, c = w1.shape
    if tuple(w2.shape) != (c, h0):
        raise ValueError(f"w2 must be ({c}, {h0}), got {tuple(w2.shape)}")
    dev = w1.device
    hp = -(-h0 // 32) * 32 if hidden_to is None else int(hidden_to)
    if hp % 32 or hp < h0:
        raise ValueError(f"hidden_to={hidden_to} must be a multiple of 32 and at least {h0}")
    ks1, ht, ct = _mlp_tiles(c, hp)
    w1p = torch.zeros(32 * ht, 16 * ks1, dtype=torch.bfloat16, device=dev)
    w1p[:h0, :c] = w1.to(torch.bfloat16)
    f1 = w1p.view(ht, 32, ks1, 2, 8).permute(0, 2, 3, 1, 4)                    # [ht, ks, h, m, j]
    w2p = torch.zeros(32 * ct, 32 * ht, dtype=torch.bfloat16, device=dev)
    w2p[:c, :h0] = (0.5 * w2.float()).to(torch.bfloat16)           # the kernel's hidden activations are 2 gelu(.) (rcx_gelu.h gelu2x_batch); halving a bf16 is exact
    unit = torch.tensor([[[_mlp_acc_unit(8 * q + j, h) for j in range(8)] for h in range(2)] for q in range(2)], device=dev)      # [q, h, j]
    f2 = w2p.view(ct, 32, ht, 32)[:, :, :, unit]                               # [ct, m, ht, q, h, j]
    f2 = f2.permute(0, 2, 3, 4, 1, 5)                                          # [ct, ht, q, h, m, j]
    # hidden-tile-major: chunk ht = its KS1 W1 fragments, then its 2 CT W2 fragments (ct, q) -- what one step of the kernels' hidden loop reads (and what the
    # large shapes stream through LDS one chunk at a time)
    f1 = f1.reshape(ht, ks1 * 512)
    f2 = f2.reshape(ct, ht, 2, 512).permute(1, 0, 2, 3).reshape(ht, ct * 2 * 512)
    wfrag = torch.cat([f1, f2], dim=1).reshape(-1).contiguous()
    bias = torch.zeros(32 * (ht + ct), dtype=torch.float32, device=dev)
    if b1 is not None:
        bias[:h0] = b1.detach().float()
    if b2 is not None:
        bias[32 * ht:32 * ht + c] = b2.detach().float()
    return wfrag, bias, 32 * ht


def _check_pack(t, dtype, numel, device, name):
    """A derived pack handed to a raw launch: the kernels read its whole extent, so a wrong size / dtype / device is refused here, not found by the GPU."""
    if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != numel or not t.is_contiguous() or t.device != device:
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of {numel} elements on {device}, got {got}")


def channel_mlp(z, x, wfrag, bias, hidden):
    """y = x + W2 gelu(W1 z + b1) + b2 in one launch (rcx_channel_mlp_fwd; model/recnext.py:157-158): z, x N x C x H x W channels_last bf16 -> y like x."""
    z = _nhwc(z, "z")
    x = _nhwc(x, "x")
    if z.shape != x.shape or z.dtype != x.dtype:
        raise ValueError("z and x must have the same shape and dtype")
    n, c, h, w = x.shape
    lib = _lib.load()
    if wfrag.dtype != torch.bfloat16 or wfrag.numel() * 2 != lib.rcx_channel_mlp_pack_bytes(c, hidden) or not wfrag.is_contiguous():
        raise ValueError("wfrag is not the pack of pack_channel_mlp for this (C, H)")
    _check_pack(bias, torch.float32, hidden + 32 * _mlp_tiles(c, hidden)[2], x.device, "bias")     # the kernel copies 32 (H/32 + CT) floats into LDS unconditionally
    _check_pack(wfrag, torch.bfloat16, wfrag.numel(), x.device, "wfrag")
    if z.device != x.device:
        raise ValueError("z and x must be on the same device")
    y = _empty_nhwc(n, c, h, w, x.dtype, x.device)
    with _on(x.device):
        rc = lib.rcx_channel_mlp_fwd(z.data_ptr(), x.data_ptr(), y.data_ptr(), wfrag.data_ptr(), bias.data_ptr(), n * h * w, c, hidden, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_channel_mlp_fwd")
    return y


def stem_supported(n, h, w, cm, co, dtype):
    """Whether rcx_stem_fwd has a kernel for a stem with CM intermediate and CO output channels on an N x 3 x H x W input (bf16 only)."""
    return dtype == torch.bfloat16 and _lib.load().rcx_stem_supported(int(n), int(h), int(w), int(cm), int(co), _DT[dtype]) > 0


def _pack_conv3x3_frags(w, b):
    """A dense 3x3 conv's (CO, CI, 3, 3) weight as bf16 matrix-core fragments and its bias zero padded to a multiple of 32: fragment (mt, ks) with ks = tap (KC / 16) + cg
    (KC = CI rounded up to 16): lane (h, m), element j = w[32 mt + m][16 cg + 8 h + j][tap] (zeros past CO / CI)."""
    co, ci = w.shape[0], w.shape[1]
    dev = w.device
    kc, mt = -(-ci // 16) * 16, -(-co // 32)
    wp = torch.zeros(32 * mt, kc, 9, dtype=torch.bfloat16, device=dev)
    wp[:co, :ci] = w.detach().reshape(co, ci, 9).to(torch.bfloat16)
    f = wp.view(mt, 32, kc // 16, 2, 8, 9).permute(0, 5, 2, 3, 1, 4)                         # [mt, tap, cg, h, m, j]
    bp = torch.zeros(32 * mt, dtype=torch.float32, device=dev)
    if b is not None:
        bp[:co] = b.detach().float()
    return f.reshape(-1).contiguous(), bp


def pack_stem(w1, b1, w2, b2):
    """The stem's two BN-folded 3x3 stride-2 convs -> (w1p, b1p, w2frag, b2p) for stem(): w1 (CM, 3, 3, 3), b1 (CM), w2 (CO, CM, 3, 3), b2 (CO).

    w1p: bf16 matrix-core fragments of the first conv (K = (dy, dx, c) padded to 32), b1p padded to a multiple of 32.  w2frag: bf16 matrix-core fragments, fragment (mt, ks) with ks = tap (KC / 16) + cg (KC = CM rounded up to 16):
    lane (h, m), element j = w2[32 mt + m][16 cg + 8 h + j][tap] (zeros past CO / CM).  b2p: zero padded to a multiple of 32."""
    cm, co = w1.shape[0], w2.shape[0]
    if tuple(w1.shape) != (cm, 3, 3, 3) or tuple(w2.shape) != (co, cm, 3, 3):
        raise ValueError(f"stem weights must be (CM, 3, 3, 3) and (CO, CM, 3, 3), got {tuple(w1.shape)} and {tuple(w2.shape)}")
    dev = w1.device
    m1 = -(-cm // 32)
    # first conv: K = (dy, dx, c) = 27 padded to 32; fragment (m1, ks), lane (h, m), element j = w1[32 m1 + m][k = 16 ks + 8 h + j]
    w1k = torch.zeros(32 * m1, 32, dtype=torch.bfloat16, device=dev)
    w1k[:cm, :27] = w1.detach().permute(0, 2, 3, 1).reshape(cm, 27).to(torch.bfloat16)                # (CM, dy, dx, c)
    w1p = w1k.view(m1, 32, 2, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1).contiguous()                   # [m1, ks, h, m, j]
    b1p = torch.zeros(32 * m1, dtype=torch.float32, device=dev)
    if b1 is not None:
        b1p[:cm] = b1.detach().float()
    w2frag, b2p = _pack_conv3x3_frags(w2, b2)
    return w1p, b1p, w2frag, b2p


def stem(x, w1p, b1p, w2frag, b2p, cm, co):
    """RecNextStem.forward in one launch (rcx_stem_fwd; model/recnext.py:134-146): x N x 3 x H x W channels_last bf16 -> N x CO x ceil(H/4) x ceil(W/4)."""
    x = _nhwc(x, "x")
    n, c, h, w = x.shape
    if c != 3:
        raise ValueError(f"the stem takes 3 input channels, got {c}")
    h2, w2_ = -(-(-(-h // 2)) // 2), -(-(-(-w // 2)) // 2)
    m1, mt = -(-cm // 32), -(-co // 32)
    _check_pack(w1p, torch.bfloat16, m1 * 2 * 512, x.device, "w1p")           # 2 KB per 32 intermediate channels (K = 27 padded to 32)
    _check_pack(b1p, torch.float32, 32 * m1, x.device, "b1p")
    _check_pack(w2frag, torch.bfloat16, _lib.load().rcx_stem_pack_bytes(cm, co) // 2, x.device, "w2frag")
    _check_pack(b2p, torch.float32, 32 * mt, x.device, "b2p")
    y = _empty_nhwc(n, co, h2, w2_, x.dtype, x.device)
    with _on(x.device):
        rc = _lib.load().rcx_stem_fwd(x.data_ptr(), y.data_ptr(), w1p.data_ptr(), b1p.data_ptr(), w2frag.data_ptr(), b2p.data_ptr(), n, h, w, cm, co, _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_stem_fwd")
    return y


def linear_attention_core_backward(qpre, kpre, v, gout, heads):
    """Gradients of linear_attention_core with respect to qpre, kpre (B, n, C) and v (N x C x h x w); dL/dpe = gout."""
    v = _nhwc(v, "v")
    gout = _nhwc(gout, "grad_output")
    b, c, h, w = v.shape
    n = h * w
    if gout.dtype != v.dtype:
        gout = gout.to(v.dtype)
    gq = torch.empty_like(qpre)
    gk = torch.empty_like(kpre)
    gv = _empty_nhwc(b, c, h, w, v.dtype, v.device)
    with _on(v.device):
        rc = _lib.load().rcx_linear_attention_bwd(qpre.data_ptr(), kpre.data_ptr(), v.data_ptr(), gout.data_ptr(),
                                                  gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), b, n, c, heads, _dt(v), _stream(v.device))
    _lib.check(rc, "rcx_linear_attention_bwd")
    return gq, gk, gv


class LinearAttentionCoreFn(torch.autograd.Function):
    """linear_attention_core with its HIP backward (rcx_linear_attention_bwd): forward and backward both through the C ABI."""

    @staticmethod
    def forward(ctx, qpre, kpre, v, pe, heads):
        out = linear_attention_core(qpre, kpre, v, pe, heads)
        ctx.save_for_backward(qpre, kpre, v)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, gout):
        qpre, kpre, v = ctx.saved_tensors
        gq, gk, gv = linear_attention_core_backward(qpre, kpre, v, gout, ctx.heads)
        return gq, gk, gv, gout, None


def linear_attention_wide_supported(b, n, cqk, cv, heads, dtype):
    """Whether the wide core (rcx_linear_attention_wide_*) takes b images of n tokens, q / k of cqk and v of cv channels in `heads` heads: head widths
    cqk / heads and cv / heads multiples of 4 from 4 to 128, in any pairing."""
    code = _DT.get(dtype)
    return code is not None and _lib.load().rcx_linear_attention_wide_supported(b, n, cqk, cv, heads, code) == 1


def _check_wide_args(fn, qpre, kpre, v, other, other_name, heads):
    """Every shape, dtype and device check of the wide core's entries, before anything is allocated or launched; raises ValueError."""
    for name, t in (("qpre", qpre), ("kpre", kpre), ("v", v), (other_name, other)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{fn}: {name} must be a tensor, got {type(t).__name__}")
    for name, t in (("qpre", qpre), ("kpre", kpre), ("v", v), (other_name, other)):
        if not t.is_cuda:
            raise ValueError(f"{fn}: {name} is on {t.device}: the wide linear-attention core runs on the GPU only (HIP kernels)")
        if t.device != v.device:
            raise ValueError(f"{fn}: {name} is on {t.device}, v on {v.device}")
    if v.dim() != 4:
        raise ValueError(f"{fn}: v must be 4-D (N, Cv, h, w), got shape {tuple(v.shape)}")
    if v.dtype not in _DT:
        raise ValueError(f"{fn}: v must be float32, bfloat16 or float16, got {v.dtype}")
    b, cv, h, w = v.shape
    n = h * w
    if qpre.dim() != 3 or qpre.shape[0] != b or qpre.shape[1] != n:
        raise ValueError(f"{fn}: qpre must be ({b}, {n}, Cqk), got {tuple(qpre.shape)}")
    cqk = qpre.shape[2]
    for name, t in (("qpre", qpre), ("kpre", kpre)):
        if tuple(t.shape) != (b, n, cqk) or not t.is_contiguous() or t.dtype != v.dtype:
            raise ValueError(f"{fn}: {name} must be a contiguous ({b}, {n}, {cqk}) tensor of {v.dtype}, got {tuple(t.shape)} {t.dtype}")
    if tuple(other.shape) != tuple(v.shape):
        raise ValueError(f"{fn}: {other_name} has shape {tuple(other.shape)}, expected v's {tuple(v.shape)}")
    if other_name == "pe" and other.dtype != v.dtype:
        raise ValueError(f"{fn}: pe must have v's dtype {v.dtype}, got {other.dtype}")
    if not isinstance(heads, int) or heads <= 0 or cqk % heads or cv % heads:
        raise ValueError(f"{fn}: heads={heads} must be a positive integer dividing Cqk={cqk} and Cv={cv}")
    if not linear_attention_wide_supported(b, n, cqk, cv, heads, v.dtype):
        raise ValueError(f"{fn}: no kernel for heads of {cqk // heads} (q / k) x {cv // heads} (v) channels: both must be multiples of 4 from 4 to 128")
    return b, n, cqk, cv, h, w


def linear_attention_wide(qpre, kpre, v, pe, heads):
    """The linear-attention core with separate q / k and v widths (rcx_linear_attention_wide_fwd; lsnet/model/recattn.py:97-109 LinearAttention3,
    and the 96-wide heads of LinearAttention1 / 2): qpre, kpre (B, n, Cqk) pre-activations; v, pe N x Cv x h x w, viewed as (B, n, Cv); returns
    channels_last like v."""
    b, n, cqk, cv, h, w = _check_wide_args("linear_attention_wide", qpre, kpre, v, pe, "pe", heads)
    v = _nhwc(v, "v")
    pe = _nhwc(pe, "pe")
    out = _empty_nhwc(b, cv, h, w, v.dtype, v.device)
    with _on(v.device):
        rc = _lib.load().rcx_linear_attention_wide_fwd(qpre.data_ptr(), kpre.data_ptr(), v.data_ptr(), pe.data_ptr(), out.data_ptr(),
                                                       b, n, cqk, cv, heads, _dt(v), _stream(v.device))
    _lib.check(rc, "rcx_linear_attention_wide_fwd")
    return out


def linear_attention_wide_backward(qpre, kpre, v, gout, heads):
    """Gradients of linear_attention_wide with respect to qpre, kpre (B, n, Cqk) and v (N x Cv x h x w, channels_last); dL/dpe = gout."""
    b, n, cqk, cv, h, w = _check_wide_args("linear_attention_wide_backward", qpre, kpre, v, gout, "grad_output", heads)
    v = _nhwc(v, "v")
    gout = _nhwc(gout, "grad_output")
    if gout.dtype != v.dtype:
        gout = gout.to(v.dtype)
    gq = torch.empty_like(qpre)
    gk = torch.empty_like(kpre)
    gv = _empty_nhwc(b, cv, h, w, v.dtype, v.device)
    with _on(v.device):
        rc = _lib.load().rcx_linear_attention_wide_bwd(qpre.data_ptr(), kpre.data_ptr(), v.data_ptr(), gout.data_ptr(),
                                                       gq.data_ptr(), gk.data_ptr(), gv.data_ptr(), b, n, cqk, cv, heads, _dt(v), _stream(v.device))
    _lib.check(rc, "rcx_linear_attention_wide_bwd")
    return gq, gk, gv


class LinearAttentionWideCoreFn(torch.autograd.Function):
    """linear_attention_wide with its HIP backward (rcx_linear_attention_wide_bwd), as LinearAttentionCoreFn: v and pe channels_last, dL/dpe = gout."""

    @staticmethod
    def forward(ctx, qpre, kpre, v, pe, heads):
        out = linear_attention_wide(qpre, kpre, v, pe, heads)
        ctx.save_for_backward(qpre, kpre, v)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, gout):
        qpre, kpre, v = ctx.saved_tensors
        gq, gk, gv = linear_attention_wide_backward(qpre, kpre, v, gout, ctx.heads)
        return gq, gk, gv, gout, None


def recconv2d_forward_train(x, wpack, bpack, level, k, mode="bilinear"):
    """Training forward: same result as recconv2d_forward, plus the saved fp32 pyramid the backward needs."""
    x = _nhwc(x)
    n, c, h, w = x.shape
    lib = _lib.load()
    dt = _dt(x)
    y = _empty_nhwc(n, c, h, w, x.dtype, x.device)
    nbytes = lib.rcx_recconv2d_train_saved_bytes(n, c, h, w, level, k)
    saved = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    with _on(x.device):
        rc = lib.rcx_recconv2d_fwd_train(x.data_ptr(), y.data_ptr(), wpack.data_ptr(),
                                         bpack.data_ptr() if bpack is not None else None, saved.data_ptr(), nbytes,
                                         n, c, h, w, level, k, _lib.MODES[mode], dt, _stream(x.device))
    _lib.check(rc, "rcx_recconv2d_fwd_train")
    return y, saved


def recconv2d_backward(x, gy, wpack, saved, level, k, mode="bilinear", need_bias=False, wflip=None, param_grads=None):
    """-> (gx like x, gwpack (level+2, k*k*C) f32, gbpack (level+2, C) f32 | None). Deterministic.
    wflip: the flipped pack from pack_recconv_params(with_flipped=True), if the caller has it (else it is made here).
    param_grads=(gws, gbs | None): level+2 preallocated contiguous (C,1,k,k) / (C) tensors of ONE dtype; the final reduction writes the parameters'
    gradients straight into them (no packed gradient, no unpack launch, no dtype copy) and (gx, None, None) is returned.
    gy may be float32 or, where the library reads it as it is (rcx_recconv2d_bwd_gy_dtype: the 56x56 / level 4 and 28x28 / level 3 blocks), x's own
    16-bit dtype; anything else is converted to float32 here."""
    _check_bwd_args("recconv2d_backward", x, shapes=[("gy", gy, x.shape)],
                    packs=[("wpack", wpack, (level + 2) * k * k * x.shape[1])] + ([("wflip", wflip, (level + 2) * k * k * x.shape[1])] if wflip is not None else []),
                    others=[("saved", saved)])
    n, c, h, w = x.shape
    lib = _lib.load()
    need = lib.rcx_recconv2d_train_saved_bytes(n, c, h, w, level, k)
    if saved.numel() * saved.element_size() < need:
        raise ValueError(f"recconv2d_backward: saved holds {saved.numel() * saved.element_size()} bytes, this problem's forward saves {need} "
                         "(recconv2d_forward_train)")
    x = _nhwc(x)
    want = lib.rcx_recconv2d_bwd_gy_dtype(n, c, h, w, level, k, _dt(x))
    gy = _nhwc(_gy_as_taken(gy, x.dtype, want), "grad_output")
    if wflip is None:
        wflip = wpack.view(level + 2, k, k, c).flip(1, 2).contiguous()
    gx = _empty_nhwc(n, c, h, w, x.dtype, x.device)
    gw = gb = None
    gw_ptrs = gb_ptrs = None
    grad_dt = 0
    if param_grads is not None:
        gws, gbs = param_grads
        ts = list(gws) + (list(gbs) if gbs is not None else [])
        if len(gws) != level + 2 or (gbs is not None and len(gbs) != level + 2) or any(t.dtype != ts[0].dtype or not t.is_contiguous() or t.device != x.device for t in ts) \
                or any(t.numel() != c * k * k for t in gws) or (gbs is not None and any(t.numel() != c for t in gbs)):
            raise ValueError("param_grads: level+2 contiguous (C,1,k,k) [and (C)] tensors of one dtype on x's device")
        grad_dt = _DT[ts[0].dtype]
        gw_ptrs = _ptr_array(list(gws))
        gb_ptrs = _ptr_array(list(gbs)) if gbs is not None else None
    else:
        gw = torch.empty_like(wpack)
        gb = torch.empty((level + 2, c), dtype=torch.float32, device=x.device) if need_bias else None
    nbytes = lib.rcx_recconv2d_bwd_workspace_bytes(n, c, h, w, level, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x.device)
    with _on(x.device):
        rc = lib.rcx_recconv2d_bwd(x.data_ptr(), gy.data_ptr(), _DT[gy.dtype], wpack.data_ptr(), wflip.data_ptr(), saved.data_ptr(),
                                   gx.data_ptr(), gw.data_ptr() if gw is not None else None, gb.data_ptr() if gb is not None else None,
                                   gw_ptrs, gb_ptrs, grad_dt,
                                   ws.data_ptr(), nbytes, n, c, h, w, level, k, _lib.MODES[mode], _dt(x), _stream(x.device))
    _lib.check(rc, "rcx_recconv2d_bwd")
    return gx, gw, gb


def recconv2d_input_backward(gy, wpack, wflip, level, k, mode="bilinear", dtype=None):
    """-> gx = dL/dx of RecConv2d (channels_last, `dtype`, default gy's dtype) for a block whose parameters want no gradient
    (rcx_recconv2d_bwd_input).  The block is linear in x: gx needs neither x nor a saved pyramid, only dL/dy and the two packs of
    pack_recconv_params(with_flipped=True); no weight gradient is formed.  Deterministic.
    gy may be float32 or, where the library reads it as it is (rcx_recconv2d_bwd_input_gy_dtype: the one-launch and tiled schedules), the
    block's own 16-bit dtype; anything else is converted to float32 here."""
    dtype = gy.dtype if dtype is None else dtype
    if dtype not in _DT:
        raise TypeError(f"recconv2d_input_backward: dtype must be float32, bfloat16 or float16, got {dtype}")
    if mode not in _lib.MODES:
        raise ValueError(f"mode must be 'bilinear' or 'nearest', got {mode!r}")
    numel = (level + 2) * k * k * gy.shape[1] if gy.dim() == 4 else 0
    _check_bwd_args("recconv2d_input_backward", gy, packs=[("wpack", wpack, numel), ("wflip", wflip, numel)])
    _require_gpu(gy, "grad_output")
    n, c, h, w = gy.shape
    lib = _lib.load()
    want = lib.rcx_recconv2d_bwd_input_gy_dtype(n, c, h, w, level, k, _DT[dtype])
    gy = _nhwc(_gy_as_taken(gy, dtype, want), "grad_output")
    gx = _empty_nhwc(n, c, h, w, dtype, gy.device)
    nbytes = lib.rcx_recconv2d_bwd_input_workspace_bytes(n, c, h, w, level, k)    # 0 for the one-launch blocks: nothing to allocate
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gy.device) if nbytes else None
    with _on(gy.device):
        rc = lib.rcx_recconv2d_bwd_input(gy.data_ptr(), _dt(gy), wpack.data_ptr(), wflip.data_ptr(), gx.data_ptr(),
                                         ws.data_ptr() if ws is not None else None, nbytes, n, c, h, w, level, k, _lib.MODES[mode], _dt(gx),
                                         _stream(gy.device))
    _lib.check(rc, "rcx_recconv2d_bwd_input")
    return gx


# Downsample.token_mixer of the T / S / B families: grouped_conv2d_supported, pack_grouped_weight, grouped_conv2d.  Written in recnext_amd/lsdown.py
# (with their guard-band cases in tests/test_ls_down_gpu.py) and part of this module's interface.
from .lsdown import grouped_conv2d, grouped_conv2d_supported, pack_grouped_weight            # noqa: E402, F401
# ... and the conv's backward for a training step (rcx_grouped_conv2d_bwd; guard-band cases in tests/test_ls_down_bwd_gpu.py)
from .lsdown import GroupedConv2dFn, grouped_conv2d_backward, grouped_conv2d_backward_supported, unpack_grouped_weight_grad      # noqa: E402, F401
# The T / S / B stem (rcx_stem3_fwd): stem3_supported, pack_stem3, stem3.  Written in recnext_amd/lsstem.py (guard-band cases in tests/test_ls_stem_gpu.py).
from .lsstem import pack_stem3, stem3, stem3_supported                                       # noqa: E402, F401
# nn.BatchNorm2d of a training step (rcx_batchnorm_*): written in recnext_amd/batchnorm.py (guard-band cases in tests/test_batchnorm_gpu.py)
from .batchnorm import BatchNormFn, batch_norm_backward, batch_norm_frozen, batch_norm_routed, batch_norm_supported, batch_norm_train      # noqa: E402, F401
# RepVGGDW of a training step as one operator (rcx_repdw_train_*): written in recnext_amd/repdw.py (guard-band cases in tests/test_repdw_gpu.py)
from .repdw import RepDwFn, repdw_train, repdw_train_backward, repdw_train_routed, repdw_train_supported      # noqa: E402, F401

# A depthwise ConvNorm of a training step as one operator (rcx_dwconv_bn_train_*): written in recnext_amd/dwbn.py (guard-band cases in
# tests/test_conv_norm_gpu.py)
from .dwbn import DwConvBnFn, dwconv_bn_train, dwconv_bn_train_backward, dwconv_bn_train_routed, dwconv_bn_train_supported      # noqa: E402, F401
# The classifier head, global average pool + linear, as one launch (rcx_pool_head_fwd, rcx_global_pool_fwd): written in recnext_amd/head.py (guard-band
# cases in tests/test_head_gpu.py)
from .head import global_pool, pack_head, pool_head, pool_head_routed, pool_head_supported      # noqa: E402, F401
# A channel mixer's BatchNorm + GELU and BatchNorm + residual of a training step (rcx_bn_act_*): written in recnext_amd/bnact.py (guard-band cases in
# tests/test_bnact_gpu.py)
from .bnact import BnAddFn, BnGeluFn, bn_act_routed, bn_act_supported, bn_add_train, bn_add_train_backward, bn_gelu_train, bn_gelu_train_backward      # noqa: E402, F401
