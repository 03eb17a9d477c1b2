"""The share-channel LSNet-style RecNeXt-T / S / B (lsnet/model/recattn_share_channel.py:8-485): recnext_t_share_channel / _s_ / _b_.

The family of recnext_amd.lsmodels with three differences (the two reference files' diff):
  * every attention has one head (:37-109): RecAttn2d on the slice at stages 0-1, LinearAttention3 (q / k of split/2, v of split channels) at
    stages >= 2 (:297) -- the token-half entries of lsmodels already compute both with ``heads = 1``;
  * in the share stage (:307-326, stage 3) every block with ``(block + 1) % (split_rate + 1) == 0`` has no slice mixer (:281-304): its token half
    is ``r = RepVGGDW(x)``, ``t = r + cat(x1s)``, x1s the slice-mixer outputs of the blocks since the last share block;
  * the stage carries that list from block to block.
A mixer block's x1 is ``t[:, :split]`` of its own token half, which the existing entries already write: the list holds views, and a share block's
token half is ONE HIP launch (``ls_share`` -> rcx_ls_share_fwd) that reads the four earlier t tensors where they lie.  No slice is copied and nothing
is concatenated.  In training mode, or when a gradient is needed, the share block runs ``_rep_train`` and ``r + torch.cat(...)`` under autograd.
Module and parameter names equal the reference's: its checkpoints load with ``strict=True``.

The binding of the entry lives here, not in ``ops``: every launching function of ``ops`` must have a row in the guard-band case table of
tests/test_guard_bands_gpu.py; this module's guard-band cases are in tests/test_ls_share_gpu.py.
"""
import ctypes
import functools

import torch
import torch.nn as nn

from . import _lib, lsmodels, ops
from .layers import DropPath
from .lsmodels import Downsample, LinearAttention3, LsRecAttn2d, RepVGGDW, _pack_dw, _rep_params, _rep_train, mlp

# lsnet/model/recattn_share_channel.py:461-485 (drop_path_rate of the non-distilled recipe; 0 with distillation)
SHARE_CONFIGS = {
    "recnext_t_share_channel": dict(embed_dim=(64, 128, 256, 512), depth=(0, 2, 8, 10), drop_path_rate=0.0),
    "recnext_s_share_channel": dict(embed_dim=(128, 256, 384, 512), depth=(0, 2, 8, 10), drop_path_rate=0.1),
    "recnext_b_share_channel": dict(embed_dim=(128, 256, 384, 512), depth=(2, 8, 8, 12), drop_path_rate=0.2),
}
_COMMON = dict(mlp_ratios=(2, 2, 2, 1.5), split_rates=(4, 4, 4, 4), share_stage=3)
MAX_SOURCES = 8                                      # rcx_ls_share_fwd takes 1 .. 8 sources


def ls_share_supported(b, h, w, c, split, n_src, dtype):
    """Whether rcx_ls_share_fwd has a kernel for a share block's token half: C and split multiples of 4, n_src * split == C, 1 .. 8 sources."""
    return dtype in ops._DT and _lib.load().rcx_ls_share_supported(b, h, w, c, split, n_src, ops._DT[dtype]) > 0


def _pixel_stride(fn, j, src):
    """Elements between two pixels of source `j`, a (B, split, H, W) tensor whose storage is pixel-major with the channels of a pixel side by side:
    `split` for a dense channels_last tensor, C for the slice ``t[:, :split]`` of a C-channel one.  Raises ValueError for any other layout."""
    b, s, h, w = src.shape
    sb, sc, sh, sw = src.stride()
    if s > 1 and sc != 1:
        raise ValueError(f"{fn}: source {j} has channel stride {sc}: the channels of a pixel must lie side by side (channels_last, or a channel slice of it)")
    p = sw if w > 1 else sh if h > 1 else sb if b > 1 else s
    if (w > 1 and sw != p) or (h > 1 and sh != w * p) or (b > 1 and sb != h * w * p):
        raise ValueError(f"{fn}: source {j} has strides {tuple(src.stride())} for shape {tuple(src.shape)}: not a pixel-major plane")
    if p < s or p % 4:
        raise ValueError(f"{fn}: source {j} has pixels {p} elements apart: at least its {s} channels and a multiple of 4")
    return p


def _check_share_args(fn, x, w_rep, b_rep, srcs):
    """Shape / dtype / device / layout checks of ls_share, before anything is allocated or launched (as ops._check_ls_args).  Returns (split, stride)."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f"{fn}: x must be a 4-D (N, C, H, W) tensor")
    if x.dtype not in ops._DT:
        raise ValueError(f"{fn}: x must be float32, bfloat16 or float16, got {x.dtype}")
    b, c, h, w = x.shape
    for name, t, numel in (("w_rep", w_rep, 9 * c), ("b_rep", b_rep, c)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.numel() != numel or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be a contiguous float32 tensor of {numel} elements")
        if t.device != x.device:
            raise ValueError(f"{fn}: {name} is on {t.device}, x on {x.device}")
    if not isinstance(srcs, (list, tuple)) or not 1 <= len(srcs) <= MAX_SOURCES:
        raise ValueError(f"{fn}: srcs must be a list of 1 .. {MAX_SOURCES} tensors")
    split = stride = None
    for j, s in enumerate(srcs):
        if not torch.is_tensor(s) or s.dim() != 4:
            raise ValueError(f"{fn}: source {j} must be a 4-D (N, split, H, W) tensor")
        if s.dtype != x.dtype or s.device != x.device:
            raise ValueError(f"{fn}: source {j} is {s.dtype} on {s.device}, x {x.dtype} on {x.device}")
        if (s.shape[0], s.shape[2], s.shape[3]) != (b, h, w):
            raise ValueError(f"{fn}: source {j} has shape {tuple(s.shape)}, x {tuple(x.shape)}: batch and plane must agree")
        if split is None:
            split = s.shape[1]
        if s.shape[1] != split:
            raise ValueError(f"{fn}: source {j} has {s.shape[1]} channels, source 0 has {split}")
    if len(srcs) * split != c:
        raise ValueError(f"{fn}: {len(srcs)} sources of {split} channels do not fill C = {c}")
    if split % 4:
        raise ValueError(f"{fn}: the sources' channel count ({split}) must be a multiple of 4")
    for j, s in enumerate(srcs):
        p = _pixel_stride(fn, j, s)
        if stride is None:
            stride = p
        if p != stride:
            raise ValueError(f"{fn}: source {j} has pixels {p} elements apart, source 0 has {stride}: one stride for all")
    ops._require_gpu(x, "x")
    return split, stride


def ls_share(x, w_rep, b_rep, srcs):
    """The token half of a share block (lsnet/model/recattn_share_channel.py:8-15, :281-283, :302-304; eval, BatchNorms folded): x (N, C, H, W)
    channels_last -> (r, t), r = RepVGGDW(x), t = r + the sources side by side along the channels, both like x.  w_rep / b_rep: the folded RepVGGDW
    ((3,3,C) / C packs).  srcs: len(srcs) tensors (N, C / len(srcs), H, W) of x's dtype, each channels_last or the leading channel slice
    ``t_prev[:, :split]`` of a channels_last tensor, read where it lies; any other layout raises ValueError.  One launch."""
    split, stride = _check_share_args("ls_share", x, w_rep, b_rep, srcs)
    b, c, h, w = x.shape
    if not ls_share_supported(b, h, w, c, split, len(srcs), x.dtype):
        raise ValueError(f"ls_share: no kernel for a {h} x {w} plane, C={c}, {len(srcs)} sources of {split} channels, {x.dtype} (ls_share_supported)")
    x = ops._nhwc(x, "x")
    r = torch.empty_like(x, memory_format=torch.channels_last)
    t = torch.empty_like(x, memory_format=torch.channels_last)
    ptrs = (ctypes.c_void_p * len(srcs))(*[s.data_ptr() for s in srcs])          # read during the call, not kept
    with ops._on(x.device):
        rc = _lib.load().rcx_ls_share_fwd(x.data_ptr(), r.data_ptr(), t.data_ptr(), w_rep.data_ptr(), b_rep.data_ptr(), ptrs, len(srcs), stride,
                                          b, h, w, c, split, ops._dt(x), ops._stream(x.device))
    _lib.check(rc, "rcx_ls_share_fwd")
    return r, t


def share_token_mixer(dim, num_heads, stage):
    """The slice mixer of a block (:297), one head everywhere: RecAttn2d at stages 0-1, LinearAttention3 at stages >= 2 (its constructor halves
    ``num_heads``: 2 gives the module's own num_heads of 1, q / k of dim/2 and v of dim channels)."""
    if stage >= 2:
        return LinearAttention3(dim, num_heads=2, stage=stage)
    return LsRecAttn2d(dim, num_heads=1, stage=stage)


class ShareChannelOperation(nn.Module):
    """:281-283; parameter-free.  The library-operator form: the HIP share block does not call it."""

    def forward(self, x, x1s):
        return x + torch.cat(list(x1s), dim=1)


class MetaNeXtBlock(lsmodels.MetaNeXtBlock):
    """A block with a slice mixer (:286-304): lsmodels' block; in the share stage it also hands its x1 = t[:, :split] (a view) to the stage's list."""
    is_share_block = False

    def __init__(self, in_channels, mlp_ratio, act_layer=nn.GELU, stage=0, block=0, drop_path=0, split_rate=4, token_mixer=None):
        super().__init__(in_channels, mlp_ratio, num_heads=1, act_layer=act_layer, stage=stage, block=block, drop_path=drop_path, split_rate=split_rate,
                         token_mixer=token_mixer or share_token_mixer)

    def forward(self, x, x1s=None):
        if self._hip_mixer():
            r, t = self.token_half(x)
        else:
            r = self.rep_mixer(x)
            t = self.token_mixer(r)
        if x1s is not None:
            x1s.append(t[:, :self.token_mixer.split_idx])
        return self._channel_half(r, t)


class ShareBlock(lsmodels.MetaNeXtBlock):
    """A share block (:289-294): keys ``rep_mixer.*`` and ``channel_mixer.*`` only.  ``hip=False`` (a model built with a token_mixer override) keeps
    it on library operators, like the override's slice mixers."""
    is_share_block = True

    def __init__(self, in_channels, mlp_ratio, act_layer=nn.GELU, drop_path=0, hip=True):
        nn.Module.__init__(self)
        self.rep_mixer = RepVGGDW(in_channels)
        self.token_mixer = ShareChannelOperation()
        self.channel_mixer = mlp(in_channels, in_channels * mlp_ratio, act_layer=act_layer)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self._pack_key = None
        self._pack = None
        self._hip = hip

    def _hip_mixer(self):
        return self._hip

    def _pack_tensors(self):
        return [t for t in self.rep_mixer.parameters()] + [t for t in self.rep_mixer.buffers()]

    def packed_params(self):
        """The float32 pack of the folded RepVGGDW, the same bits as a mixer block's."""
        key = tuple((t.data_ptr(), t._version, t.dtype, t.device) for t in self._pack_tensors())
        if key != self._pack_key:
            with torch.no_grad():
                self._pack = tuple(_pack_dw(*_rep_params(self.rep_mixer)))
            self._pack_key = key
        return self._pack

    def token_half(self, x, x1s):
        """(r, t) as one HIP launch; in training mode or when a gradient is needed: _token_half_train.  A CPU tensor or a shape without a kernel raises."""
        if not x1s:
            raise ValueError("a share block needs the slice-mixer outputs of the blocks before it (x1s is empty)")
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or any(s.requires_grad for s in x1s)
                                                          or any(p.requires_grad for p in self.parameters()))):
            return self._token_half_train(x, x1s)
        if not x.is_cuda:
            raise RuntimeError("recnext_amd's share-channel RecNeXt-T / S / B token half runs on the GPU only (HIP kernels); the CPU formulation is "
                               "tests/ls_share_eager.py")
        b, c, h, w = x.shape
        split = x1s[0].shape[1]
        if not ls_share_supported(b, h, w, c, split, len(x1s), x.dtype):
            raise NotImplementedError(f"share block: no kernel for a {h} x {w} plane of {c} channels with {len(x1s)} sources of {split} ({x.dtype})")
        return ls_share(x, *self.packed_params(), list(x1s))

    def _token_half_train(self, x, x1s):
        if not x.is_cuda:
            raise NotImplementedError("training the share-channel RecNeXt-T / S / B runs on the GPU only (HIP kernels); the CPU formulation is "
                                      "tests/ls_share_eager.py")
        x = x.contiguous(memory_format=torch.channels_last)
        r = _rep_train(self.rep_mixer, x)
        t = r + torch.cat([s.to(r.dtype) for s in x1s], dim=1)
        return r, t.contiguous(memory_format=torch.channels_last)

    def forward(self, x, x1s):
        if self._hip_mixer():
            r, t = self.token_half(x, x1s)
        else:
            r = self.rep_mixer(x)
            t = self.token_mixer(r, x1s)
        return self._channel_half(r, t)


class RecNextStage(nn.Module):
    """:307-326.  In the share stage the forward carries the list x1s: a mixer block appends, a share block consumes and the list is cleared."""

    def __init__(self, in_channels, out_channels, depth, mlp_ratio, num_heads=1, act_layer=nn.GELU, downsample=True, stage=0, split_rate=4,
                 drop_path_rates=None, token_mixer=None, share_stage=3):
        super().__init__()
        drop_path_rates = drop_path_rates or [0.0] * depth
        self.is_share_stage = stage >= share_stage
        self.downsample = Downsample(in_channels, out_channels, mlp_ratio, act_layer=act_layer, stage=stage,
                                     drop_path=drop_path_rates[0] if depth else 0.0) if downsample else nn.Identity()
        blocks = []
        for i in range(depth):
            if self.is_share_stage and (i + 1) % (split_rate + 1) == 0:
                blocks.append(ShareBlock(out_channels, mlp_ratio, act_layer=act_layer, drop_path=drop_path_rates[i], hip=token_mixer is None))
            else:
                blocks.append(MetaNeXtBlock(out_channels, mlp_ratio, act_layer=act_layer, stage=stage, block=i, drop_path=drop_path_rates[i],
                                            split_rate=split_rate, token_mixer=token_mixer))
        self.blocks = nn.ModuleList(blocks) if self.is_share_stage else nn.Sequential(*blocks)

    def forward(self, x):
        x = self.downsample(x)
        if not self.is_share_stage:
            return self.blocks(x)
        x1s = []
        for block in self.blocks:
            x = block(x, x1s)
            if block.is_share_block:
                x1s.clear()
        return x


class RecNext(lsmodels.RecNext):
    """:329-395: lsmodels' skeleton with this family's stages."""

    def __init__(self, share_stage=3, **kwargs):
        kwargs.pop("num_heads", None)                          # the family's constructors take none (:37-109)
        n = len(kwargs.get("embed_dim", (48,)))
        super().__init__(num_heads=(1,) * n, stage_factory=functools.partial(RecNextStage, share_stage=share_stage), **kwargs)


def create_model(name, distillation=False, token_mixer=None, **overrides):
    """recnext_t_share_channel / _s_ / _b_ (:461-485).  ``token_mixer(dim, num_heads, stage)`` replaces the slice mixer and keeps the share blocks on
    library operators (tests host tests/ls_share_eager.py's restatement)."""
    cfg = dict(_COMMON, **SHARE_CONFIGS[name])
    if distillation:
        cfg["drop_path_rate"] = 0.0
    cfg.update(overrides)
    return RecNext(distillation=distillation, token_mixer=token_mixer, **cfg)


def mixer_shapes(name, resolution=224):
    """[(stage, H, W, C, split, heads, kind, blocks)] of every block's token half in one forward (kind 'recattn' | 'la3' | 'share'; a share row counts
    the stage's share blocks and has heads 0).  `resolution`: the input's side, or its (H, W)."""
    cfg = dict(_COMMON, **SHARE_CONFIGS[name])
    sides = [resolution, resolution] if isinstance(resolution, int) else [int(v) for v in resolution]
    if len(sides) != 2:
        raise ValueError("resolution must be an int or an (H, W) pair")
    for _ in range(3):
        sides = [(v + 1) // 2 for v in sides]                   # the stem: three 3x3 stride-2 convs
    out = []
    for i, (c, d) in enumerate(zip(cfg["embed_dim"], cfg["depth"])):
        if i:
            sides = [(v + 1) // 2 for v in sides]               # Downsample: 5x5 stride 2, padding 2
        if d:
            rate = cfg["split_rates"][i]
            shared = d // (rate + 1) if i >= cfg["share_stage"] else 0
            out.append((i, sides[0], sides[1], c, c // rate, 1, "la3" if i >= 2 else "recattn", d - shared))
            if shared:
                out.append((i, sides[0], sides[1], c, c // rate, 0, "share", shared))
    return out
