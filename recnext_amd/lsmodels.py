"""The LSNet-style RecNeXt-T / S / B (lsnet/model/recattn.py:8-466): RecAttn2d applied to a quarter of the channels.

Each block computes ``r = RepVGGDW(x)`` (:8-34), ``t = cat(mixer(r[:, :C/4]), r[:, C/4:])`` (:226-237) and returns ``r + MLP(t)`` (:240-251); the
mixer is RecAttn2d at stages 0-2 (:115-127) and LinearAttention3 at stage 3 (:89-112).  Module and parameter names equal the reference's, so its
checkpoints load with ``strict=True`` and ``models.replace_batchnorm`` gives the keys of its ``RecNext.fuse()``.

The token half ``x -> (r, t)`` of every block is ONE HIP entry (two launches: ``ops.ls_recattn`` / ``ops.ls_la3``), BatchNorms folded into float32
packs whether or not ``replace_batchnorm`` has run; where that entry's support query says no (planes above 224 x 224's), the tiled entry
(``ops.ls_recattn_tiled`` / ``ops.ls_la3_tiled``: the same function on any H x W, three or four launches) takes the block, and behind it the HIP
depthwise conv and the library's ``RecAttn2d`` on a contiguous slice remain for heads of at most 64 channels.  A forward in training mode or one that needs a gradient takes the training
form (``_token_half_train``): BatchNorms on batch statistics under autograd, nothing folded, the depthwise convs and the attention cores with HIP
forward and backward kernels -- ``RecAttn2d``'s own training branch at stages 0-2 (the 96-wide heads of S / B's stage 2 on the wide core,
``rcx_linear_attention_wide_*``) and ``LinearAttention3.forward`` at stage 3 (q / k of s/2 and v of s channels: the wide core) -- and library GEMMs
for the 1x1 projections.  A CPU tensor raises.  Downsample's grouped 5x5 stride-2 conv (:254-263) is ONE HIP launch (``ops.grouped_conv2d``) in an
inference forward after ``models.use_hip_downsample`` (opt-in; ``speed.build_inference_model`` calls it); in training, where a gradient is needed and
on a CPU tensor it stays the library's conv.  The stem's three convs and their GELUs are TWO HIP launches (``ops.stem3``) in a bf16 inference forward after
``models.use_fused_stem`` (``speed.build_inference_model`` calls it); in training, in float32 / fp16, where a gradient is needed and on a CPU tensor the stem stays
the library's.  The classifier is a PyTorch-ROCm library operator.

RecAttn2d's ``stage -> LinearAttention1 | 2`` label (:119) is cosmetic: the two are the same function (the reference asserts it, :481-501).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import bnact                 # after ops, which re-exports from it
from ._trainop import gpu_tensor_ok
from .batchnorm import bump, norm_fusable
from .layers import ConvNorm as _ConvNorm
from .layers import DropPath
from .dwconv import DwConvFn
from .recattn import RecAttn2d, _conv_norm_train, _folded, head_dim_supported

# lsnet/model/recattn.py:441-466 (drop_path_rate of the non-distilled recipe; 0 with distillation)
LS_CONFIGS = {
    "recnext_t": dict(embed_dim=(64, 128, 256, 512), depth=(0, 2, 8, 10), drop_path_rate=0.0),
    "recnext_s": dict(embed_dim=(128, 256, 384, 512), depth=(0, 2, 8, 10), drop_path_rate=0.1),
    "recnext_b": dict(embed_dim=(128, 256, 384, 512), depth=(2, 8, 8, 12), drop_path_rate=0.2),
}
_COMMON = dict(mlp_ratios=(2, 2, 2, 1.5), num_heads=(1, 1, 1, 2), split_rates=(4, 4, 4, 4))


def ConvNorm(*args, **kwargs):
    """The family's ConvNorm: the reference's has a conv bias (:130-146), unlike the M / A families'."""
    kwargs.setdefault("bias", True)
    return _ConvNorm(*args, **kwargs)


def _fold_rep(lk, sk):
    """RepVGGDW.fuse (:17-34) in float32: lk + zero-padded sk + identity at the centre tap.  Both the fuse and the HIP pack use it, so a folded
    and an unfolded model run on bit-identical packs."""
    wl, bl = _folded(lk)
    ws, bs = _folded(sk)
    wl, ws = wl.float(), ws.float()
    ident = F.pad(torch.ones(wl.shape[0], wl.shape[1], 1, 1, device=wl.device), [1, 1, 1, 1])
    w = wl + F.pad(ws, [1, 1, 1, 1]) + ident
    zero = torch.zeros(wl.shape[0], device=wl.device)
    b = (zero if bl is None else bl.float()) + (zero if bs is None else bs.float())
    return w, b


class RepVGGDW(nn.Module):
    def __init__(self, in_channels):
        super().__init__()
        self.lk = ConvNorm(in_channels, in_channels, kernel_size=3, padding=1, groups=in_channels)
        self.sk = ConvNorm(in_channels, in_channels, kernel_size=1, padding=0, groups=in_channels)

    def forward(self, x):
        return self.lk(x) + self.sk(x) + x

    @torch.no_grad()
    def fuse(self):
        w, b = _fold_rep(self.lk, self.sk)
        conv = self.lk.conv
        out = nn.Conv2d(conv.in_channels, conv.out_channels, 3, padding=1, groups=conv.groups, bias=True, device=w.device, dtype=conv.weight.dtype)
        out.weight.copy_(w)
        out.bias.copy_(b)
        return out


def _rep_train(m, x):
    """RepVGGDW (or its fused nn.Conv2d) in a training step: lk = HIP depthwise 3x3 (biased) + its BatchNorm, sk = the depthwise 1x1 as a per-channel
    affine x w + b + its BatchNorm, then lk + sk + x (:8-15).  Batch statistics in train mode, nothing folded."""
    if isinstance(m, nn.Conv2d):
        return DwConvFn.apply(x, m.weight, m.bias, 1)
    if m.__dict__.get("_fused_rep_train") and _rep_fused_ok(m, x):
        return _rep_fused(m, x)
    lk = _conv_norm_train(m.lk, x, 1)
    sk = m.sk if isinstance(m.sk, nn.Conv2d) else m.sk.conv
    c = x.shape[1]
    y = x * sk.weight.view(1, c, 1, 1)
    if sk.bias is not None:
        y = y + sk.bias.view(1, c, 1, 1)
    if not isinstance(m.sk, nn.Conv2d):
        y = m.sk.norm(y)
    return lk + y + x


def _rep_fused_ok(m, x):
    """Whether a RepVGGDW that models.use_fused_rep_train marked runs this call on ops.RepDwFn (the conditions of that function's docstring)."""
    if not (gpu_tensor_ok(x) and x.numel() > x.shape[1]):
        return False
    if not isinstance(m, RepVGGDW) or isinstance(m.lk, nn.Conv2d) or isinstance(m.sk, nn.Conv2d):
        return False
    for cn in (m.lk, m.sk):
        conv = cn.conv
        if conv.bias is None or conv.weight.dtype != torch.float32 or conv.bias.dtype != torch.float32 or not norm_fusable(cn.norm):
            return False
    if (m.lk.norm.running_mean is None) != (m.sk.norm.running_mean is None):
        return False
    n, c, h, w = x.shape
    return ops.repdw_train_supported(n, h, w, c, x.dtype, measured_only=m.__dict__["_fused_rep_train"] != "all")


def _rep_fused(m, x):
    na, nb = m.lk.norm, m.sk.norm
    return ops.RepDwFn.apply(ops._nhwc(x), m.lk.conv.weight, m.lk.conv.bias, na.weight, na.bias, m.sk.conv.weight, m.sk.conv.bias, nb.weight, nb.bias,
                             *bump(na), *bump(nb), na.momentum, na.eps, nb.momentum, nb.eps)


def _rep_params(m):
    """(weight (C,1,3,3), bias (C)) in float32 of a RepVGGDW or of its fused nn.Conv2d."""
    if isinstance(m, nn.Conv2d):
        return m.weight.float(), m.bias.float()
    return _fold_rep(m.lk, m.sk)


class LsRecAttn2d(RecAttn2d):
    """The library's RecAttn2d with the family's biased ConvNorms (keys ``down.0.conv.bias`` ... as :115-127).  Stage 0 carries the label
    LinearAttention1, stages 1-2 LinearAttention2 (:119); the function is the same."""

    def __init__(self, dim, num_heads, kernel_size=5, stage=1, mode="nearest"):
        super().__init__(dim, num_heads, kernel_size=kernel_size, stage=stage, mode=mode)
        p = kernel_size // 2
        self.down[0] = ConvNorm(dim, dim, kernel_size=kernel_size, padding=p, stride=2, groups=dim)
        la = self.down[1]
        la.variant = 1 if stage == 0 else 2
        la.qk = ConvNorm(dim, dim * 2, kernel_size=1, groups=2)
        la.pe = ConvNorm(dim, dim, kernel_size=3, padding=1, groups=dim)
        self.conv = ConvNorm(dim, dim, kernel_size=kernel_size, padding=p, groups=dim)

    def _tensors(self):
        out = super()._tensors()
        for m in (self.down[0], self.conv, self.down[1].qk, self.down[1].pe):      # the conv biases, which the A family does not have
            if not isinstance(m, nn.Conv2d) and m.conv.bias is not None:
                out.append(m.conv.bias)
        return out


class LinearAttention3(nn.Module):
    """:89-112.  ``num_heads`` is half the constructor's; q and k take ``dim / 2`` channels of the full 1x1 ``qk`` each, v is the input."""

    def __init__(self, dim, num_heads, **kwargs):
        super().__init__()
        self.num_heads = num_heads // 2
        self.head_dim = dim // self.num_heads // 2
        self.qk = ConvNorm(dim, dim, kernel_size=1, groups=1)
        self.pe = ConvNorm(dim, dim, kernel_size=3, padding=1, groups=dim)

    def forward(self, x):
        """The training-step form (MetaNeXtBlock's token half calls it; inference runs inside ops.ls_la3): the full 1x1 `qk` as one GEMM on the
        token-major view + the module's BatchNorm, q = its channels [0, s/2), k = [s/2, s), v = x, pe = HIP depthwise 3x3 + BatchNorm, then the
        wide core with its HIP backward (rcx_linear_attention_wide_fwd / _bwd)."""
        b, c, h, w = x.shape
        n = h * w
        if not x.is_cuda:
            raise RuntimeError("recnext_amd's LinearAttention3 runs on the GPU only (HIP kernels); the CPU formulation is tests/ls_eager.py")
        if c % 2 or x.dtype not in ops._DT or not ops.linear_attention_wide_supported(b, n, c // 2, c, self.num_heads, x.dtype):
            raise NotImplementedError(f"LinearAttention3: the HIP core takes heads of 4 .. 128 channels in fours; got dim {c}, {self.num_heads} heads, {x.dtype}")
        m = self.qk
        conv = m if isinstance(m, nn.Conv2d) else m.conv
        y = F.linear(x.permute(0, 2, 3, 1).reshape(b * n, c), conv.weight[:, :, 0, 0], conv.bias)
        y = y.view(b, h, w, c).permute(0, 3, 1, 2)
        if not isinstance(m, nn.Conv2d):
            y = m.norm(y)
        tok = y.to(x.dtype).permute(0, 2, 3, 1).reshape(b, n, c)        # under autocast the GEMM answers in the autocast type: the core takes x's
        qpre, kpre = tok[..., :c // 2].contiguous(), tok[..., c // 2:].contiguous()
        pe = _conv_norm_train(self.pe, x, 1).to(x.dtype)
        return ops.LinearAttentionWideCoreFn.apply(qpre, kpre, x.contiguous(memory_format=torch.channels_last), pe, self.num_heads)

    def extra_repr(self):
        return f"num_heads={self.num_heads}, head_dim={self.head_dim}"


def default_token_mixer(dim, num_heads, stage):
    """The slice mixer of a block (:222): RecAttn2d at stages 0-2, LinearAttention3 at stage 3."""
    if stage >= 3:
        return LinearAttention3(dim, num_heads=num_heads, stage=stage)
    return LsRecAttn2d(dim, num_heads=num_heads, stage=stage)


class PartialChannelOperation(nn.Module):
    def __init__(self, in_channels, attn, split_rate=4):
        super().__init__()
        assert in_channels % split_rate == 0, "in_channels must be divisible by split_rate"
        self.split_idx = in_channels // split_rate
        self.attn = attn

    def forward(self, x):
        return torch.cat([self.attn(x[:, :self.split_idx]), x[:, self.split_idx:]], dim=1)


def mlp(in_channels, hidden_channels, act_layer=nn.GELU):
    hidden_channels = int(hidden_channels)
    return nn.Sequential(ConvNorm(in_channels, hidden_channels, kernel_size=1), act_layer(), ConvNorm(hidden_channels, in_channels, kernel_size=1))


def _pack_dw(w, b):
    return ops.pack_dw_weight(w.float().contiguous()), ops.pack_bias(b.float().contiguous())


class MetaNeXtBlock(nn.Module):
    """r = rep_mixer(x); return r + drop_path(channel_mixer(token_mixer(r))) (:240-251).  With the family's own slice mixers the token half runs on HIP."""

    def __init__(self, in_channels, mlp_ratio, num_heads=2, act_layer=nn.GELU, stage=0, block=0, drop_path=0, split_rate=4, token_mixer=None):
        super().__init__()
        self.rep_mixer = RepVGGDW(in_channels)
        attn = (token_mixer or default_token_mixer)(in_channels // split_rate, num_heads, stage)
        self.token_mixer = PartialChannelOperation(in_channels, attn, split_rate=split_rate)
        self.channel_mixer = mlp(in_channels, in_channels * mlp_ratio, act_layer=act_layer)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self._pack_key = None
        self._pack = None

    def _hip_mixer(self):
        return isinstance(self.token_mixer, PartialChannelOperation) and type(self.token_mixer.attn) in (LsRecAttn2d, LinearAttention3)

    def _pack_tensors(self):
        out = [t for t in self.rep_mixer.parameters()] + [t for t in self.rep_mixer.buffers()]
        out += [t for t in self.token_mixer.attn.parameters()] + [t for t in self.token_mixer.attn.buffers()]
        return out

    def packed_params(self):
        """Float32 packs of the token half: the folded RepVGGDW, then the slice mixer's folded convs (q / k rows transposed)."""
        key = tuple((t.data_ptr(), t._version, t.dtype, t.device) for t in self._pack_tensors())
        if key != self._pack_key:
            with torch.no_grad():
                attn = self.token_mixer.attn
                s = self.token_mixer.split_idx
                pack = list(_pack_dw(*_rep_params(self.rep_mixer)))
                if isinstance(attn, LinearAttention3):
                    wqk, bqk = _folded(attn.qk)                    # (s, s, 1, 1): rows [0, s/2) = q, [s/2, s) = k
                    wqk = wqk[:, :, 0, 0].float()
                    bqk = bqk.float()
                    pack += [wqk[:s // 2].t().contiguous(), bqk[:s // 2].contiguous(), wqk[s // 2:].t().contiguous(), bqk[s // 2:].contiguous()]
                    pack += list(_pack_dw(*_folded(attn.pe)))
                else:
                    la = attn.down[1]
                    pack += list(_pack_dw(*_folded(attn.down[0])))
                    wqk, bqk = _folded(la.qk)                      # (2s, s/2, 1, 1): rows [0, s) = q from channels [0, s/2), [s, 2s) = k from [s/2, s)
                    wqk = wqk[:, :, 0, 0].float()
                    bqk = bqk.float()
                    pack += [wqk[:s].t().contiguous(), bqk[:s].contiguous(), wqk[s:].t().contiguous(), bqk[s:].contiguous()]
                    pack += list(_pack_dw(*_folded(la.pe)))
                    pack += list(_pack_dw(*_folded(attn.conv)))
                self._pack = tuple(pack)
            self._pack_key = key
        return self._pack

    def token_half(self, x):
        """(r, t) on HIP: the one-workgroup entry (two launches) where its support query says yes, else the tiled entry (any plane size), else the
        HIP depthwise conv + the library's RecAttn2d on a contiguous slice (heads of at most 64 channels; no registered model reaches it); raises
        otherwise.  In training mode or when a gradient is needed: _token_half_train."""
        attn = self.token_mixer.attn
        s = self.token_mixer.split_idx
        b, c, h, w = x.shape
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return self._token_half_train(x)
        if not x.is_cuda:
            raise RuntimeError("recnext_amd's RecNeXt-T / S / B token mixer runs on the GPU only (HIP kernels); the CPU formulation is tests/ls_eager.py")
        if isinstance(attn, LinearAttention3):
            if ops.ls_la3_supported(b, h, w, c, s, attn.num_heads, x.dtype):
                return ops.ls_la3(x, *self.packed_params(), s, attn.num_heads)
            if ops.ls_la3_tiled_supported(b, h, w, c, s, attn.num_heads, x.dtype):
                return ops.ls_la3_tiled(x, *self.packed_params(), s, attn.num_heads)
            raise NotImplementedError(f"RecNeXt-T / S / B LinearAttention3: no kernel for a {h} x {w} plane of {c} channels (slice {s}, {attn.num_heads} heads, {x.dtype})")
        heads = attn.down[1].num_heads
        if ops.ls_recattn_supported(b, h, w, c, s, heads, x.dtype):
            return ops.ls_recattn(x, *self.packed_params(), s, heads)
        if ops.ls_recattn_tiled_supported(b, h, w, c, s, heads, x.dtype):
            return ops.ls_recattn_tiled(x, *self.packed_params(), s, heads)
        if s % heads == 0 and head_dim_supported(s // heads) and x.dtype in ops._DT:
            wr, br = self.packed_params()[:2]
            r = ops.dwconv2d(x, wr, br, k=3, stride=1)
            t = torch.cat([attn(r[:, :s].contiguous(memory_format=torch.channels_last)), r[:, s:]], dim=1)
            return r, t.contiguous(memory_format=torch.channels_last)
        raise NotImplementedError(f"RecNeXt-T / S / B RecAttn2d: no kernel for a {h} x {w} plane of {c} channels (slice {s}, {heads} heads of {s // heads}, {x.dtype})")

    def _token_half_train(self, x):
        """(r, t) in a training step or a forward that needs a gradient: RepVGGDW (_rep_train), the slice mixer's own training form, the concatenation
        under autograd; channels_last kept."""
        if not x.is_cuda:
            raise NotImplementedError("training RecNeXt-T / S / B runs on the GPU only (HIP kernels); the CPU formulation is tests/ls_eager.py")
        s = self.token_mixer.split_idx
        x = x.contiguous(memory_format=torch.channels_last)
        r = _rep_train(self.rep_mixer, x)
        mixed = self.token_mixer.attn(r[:, :s].contiguous(memory_format=torch.channels_last))
        t = torch.cat([mixed.to(r.dtype), r[:, s:]], dim=1)
        return r, t.contiguous(memory_format=torch.channels_last)

    def forward(self, x):
        if self._hip_mixer():
            r, t = self.token_half(x)
        else:
            r = self.rep_mixer(x)
            t = self.token_mixer(r)
        return self._channel_half(r, t)

    def _channel_half(self, r, t):
        """r + drop_path(channel_mixer(t)): the block's tail, whatever made (r, t)."""
        fused = self.__dict__.get("_fused_mlp")
        if fused is not None and not self.training and fused.usable(self.channel_mixer, t, r):
            return fused(t, r)                              # r + channel_mixer(t) in one launch (models.use_fused_mlp)
        if bnact.ATTR in self.channel_mixer.__dict__:       # models.use_fused_mixer_norms_train: the two norms with their epilogues in a training forward
            mode = bnact.mixer_ready(self.channel_mixer, t)
            if mode is not None:
                return bnact.run_mixer(self.channel_mixer, t, r, self.drop_path, mode)
        return r + self.drop_path(self.channel_mixer(t))


class Downsample(nn.Module):
    """:254-263.  After ``models.use_hip_downsample`` an inference forward runs ``token_mixer`` -- the grouped 5x5 stride-2 ConvNorm with
    gcd(Cin, Cout) groups -- as ONE HIP launch (``ops.grouped_conv2d``) on a float32 pack folded by ``_folded``, the same for the ConvNorm and its
    ``replace_batchnorm``ed nn.Conv2d.  Decided per call (``_hip_conv``); everything else keeps the library operators."""

    def __init__(self, in_channels, out_channels, mlp_ratio=2, act_layer=nn.GELU, kernel_size=5, stage=0, drop_path=0):
        super().__init__()
        self.token_mixer = ConvNorm(in_channels, out_channels, kernel_size=kernel_size, padding=(kernel_size - 1) // 2, stride=2,
                                    groups=math.gcd(in_channels, out_channels))
        self.channel_mixer = mlp(out_channels, out_channels * mlp_ratio, act_layer=act_layer)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self._hip = False                       # set by models.use_hip_downsample; a plain attribute, so the state_dict keys stay
        self._pack_key = None
        self._pack = None

    def _conv(self):
        """token_mixer's nn.Conv2d if token_mixer is still this family's ConvNorm or its fused nn.Conv2d, else None (a replaced child)."""
        tm = self.token_mixer
        if isinstance(tm, nn.Conv2d):
            return tm
        if isinstance(tm, _ConvNorm) and isinstance(tm.conv, nn.Conv2d) and isinstance(tm.norm, nn.BatchNorm2d):
            return tm.conv
        return None

    def _hip_conv(self, x):
        """Whether this call takes the HIP launch: rerouted, eval mode, a GPU tensor, no gradient wanted anywhere, no autocast, and a kernel for the shape."""
        if not self.__dict__.get("_hip") or self.training or not x.is_cuda or x.dim() != 4 or torch.is_autocast_enabled():
            return False
        conv = self._conv()
        if conv is None or conv.kernel_size != (5, 5) or conv.stride != (2, 2) or conv.padding != (2, 2) or conv.dilation != (1, 1) \
                or conv.padding_mode != "zeros" or conv.in_channels != x.shape[1]:
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.token_mixer.parameters())):
            return False
        n, _, h, w = x.shape
        return ops.grouped_conv2d_supported(n, h, w, conv.in_channels, conv.out_channels, conv.groups, 5, 2, x.dtype)

    def packed_params(self):
        """(wpack, bias): the folded token_mixer as ops.grouped_conv2d takes it, rebuilt when a parameter or buffer changes."""
        tm = self.token_mixer
        key = tuple((t.data_ptr(), t._version, t.dtype, t.device) for t in list(tm.parameters()) + list(tm.buffers()))
        if key != self.__dict__.get("_pack_key"):              # (a whole-model pickle from before the reroute has no such attribute)
            with torch.no_grad():
                w, b = _folded(tm)
                self._pack = (ops.pack_grouped_weight(w), None if b is None else b.detach().float().contiguous())
            self._pack_key = key
        return self._pack

    def forward(self, x):
        if self._hip_conv(x):
            x = ops.grouped_conv2d(x, *self.packed_params(), self._conv().groups)
        else:
            x = self.token_mixer(x)
        fused = self.__dict__.get("_fused_mlp")
        if fused is not None and not self.training and fused.usable(self.channel_mixer, x, x):
            return fused(x, x)
        if bnact.ATTR in self.channel_mixer.__dict__:
            mode = bnact.mixer_ready(self.channel_mixer, x)
            if mode is not None:
                return bnact.run_mixer(self.channel_mixer, x, x, self.drop_path, mode)
        return x + self.drop_path(self.channel_mixer(x))


class RecNextStem(nn.Module):
    def __init__(self, in_channels, out_channels, act_layer=nn.GELU, kernel_size=3, stride=2, additional_activation=False):
        super().__init__()
        kw = dict(kernel_size=kernel_size, stride=stride, padding=(kernel_size - 1) // 2)
        self.stem = nn.Sequential(ConvNorm(in_channels, out_channels // 4, **kw), act_layer(), ConvNorm(out_channels // 4, out_channels // 2, **kw), act_layer(),
                                  ConvNorm(out_channels // 2, out_channels, **kw), act_layer() if additional_activation else nn.Identity())

    def forward(self, x):
        fused = self.__dict__.get("_fused_stem")
        if fused is not None and not self.training and fused.usable(self.stem, x):
            return fused(x)                             # two launches (models.use_fused_stem)
        if bnact.ATTR in self.__dict__:                 # models.use_fused_mixer_norms_train: ConvNorm -> GELU on BnGeluFn in a training forward
            mode = bnact.stem_ready(self, x)
            if mode is not None:
                return bnact.run_stem(self.stem, x, mode)
        return self.stem(x)


class RecNextStage(nn.Module):
    def __init__(self, in_channels, out_channels, depth, mlp_ratio, num_heads=2, act_layer=nn.GELU, downsample=True, stage=0, split_rate=4,
                 drop_path_rates=None, token_mixer=None):
        super().__init__()
        drop_path_rates = drop_path_rates or [0.0] * depth
        self.downsample = Downsample(in_channels, out_channels, mlp_ratio, act_layer=act_layer, stage=stage,
                                     drop_path=drop_path_rates[0] if depth else 0.0) if downsample else nn.Identity()
        self.blocks = nn.Sequential(*[MetaNeXtBlock(out_channels, mlp_ratio, num_heads=num_heads, act_layer=act_layer, stage=stage, block=i,
                                                    drop_path=drop_path_rates[i], split_rate=split_rate, token_mixer=token_mixer) for i in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class RecNext(nn.Module):
    def __init__(self, in_chans=3, embed_dim=(48,), depth=(2,), mlp_ratios=(2,), num_heads=(2,), global_pool="avg", num_classes=1000, act_layer=nn.GELU,
                 distillation=False, split_rates=(4,), drop_rate=0.0, drop_path_rate=0.0, token_mixer=None, stage_factory=None):
        from .models import RecNextClassifier
        super().__init__()
        stage_factory = stage_factory or RecNextStage        # RecNextStage's signature (recnext_amd.lsshare brings its own stage)
        self.global_pool = global_pool
        self.embed_dim = tuple(embed_dim)
        self.num_classes = num_classes
        in_channels = embed_dim[0]
        self.stem = RecNextStem(in_chans, in_channels, act_layer=act_layer, additional_activation=depth[0] == 0)
        dpr = [x.tolist() for x in torch.linspace(0, drop_path_rate, sum(depth)).split(list(depth))]
        stages = []
        for i in range(len(embed_dim)):
            stages.append(stage_factory(in_channels, embed_dim[i], depth[i], mlp_ratio=mlp_ratios[i], num_heads=num_heads[i], act_layer=act_layer,
                                        downsample=i != 0, stage=i, split_rate=split_rates[i], drop_path_rates=dpr[i], token_mixer=token_mixer))
            in_channels = embed_dim[i]
        self.stages = nn.Sequential(*stages)
        self.num_features = embed_dim[-1]
        self.head_drop = nn.Dropout(drop_rate)
        self.head = RecNextClassifier(embed_dim[-1], num_classes, distillation)

    def forward_features(self, x):
        return self.stages(self.stem(x))

    def forward_head(self, x):
        fused = self.__dict__.get("_fused_head")
        if fused is not None and fused.usable(self, x):
            return fused(x)                             # global pool + linear as one launch (models.use_fused_head)
        if self.global_pool == "avg":
            x = x.mean((2, 3))
        return self.head(self.head_drop(x))

    def forward(self, x):
        return self.forward_head(self.forward_features(x))


def create_model(name, distillation=False, token_mixer=None, **overrides):
    """recnext_t / _s / _b (:441-466).  ``token_mixer(dim, num_heads, stage)`` replaces the slice mixer (tests host tests/ls_eager.py's restatement)."""
    cfg = dict(_COMMON, **LS_CONFIGS[name])
    if distillation:
        cfg["drop_path_rate"] = 0.0
    cfg.update(overrides)
    return RecNext(distillation=distillation, token_mixer=token_mixer, **cfg)


def mixer_shapes(name, resolution=224):
    """[(stage, H, W, C, split, heads, kind, blocks)] of every block's token half in one forward (kind 'recattn' | 'la3'; heads as the entries take them).
    `resolution`: the input's side, or its (H, W)."""
    cfg = dict(_COMMON, **LS_CONFIGS[name])
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
            split = c // cfg["split_rates"][i]
            kind = "la3" if i >= 3 else "recattn"
            heads = cfg["num_heads"][i] // 2 if kind == "la3" else cfg["num_heads"][i]
            out.append((i, sides[0], sides[1], c, split, heads, kind, d))
    return out
