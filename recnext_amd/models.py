"""timm-free model skeleton that hosts the token mixers: RecNeXt-M0..M5 (RecConv2d) and A0..A5 (RecAttn2d).

Restates the *structure* of model/recnext.py:125-287 and model/recattn.py:139-300 (stem, four stages of
MetaNeXt blocks, strided-depthwise Downsample, two-headed classifier) with the reference's module
and parameter names, so ``state_dict`` keys -- and therefore released checkpoints -- are interchangeable.
Everything here is ordinary PyTorch-ROCm plumbing (1x1 convs, BN, GELU run on MIOpen/hipBLASLt);
the only arithmetic owned by this repository is inside ``token_mixer``.

``token_mixer`` factories are injectable so tests / the CPU baseline can host the oracle's ATen
restatement in the same skeleton; the default is always the HIP module.
"""
import torch
import torch.nn as nn

from . import ops
from . import bnact                 # after ops, which re-exports from it
from .layers import ConvNorm, DropPath, NormLinear
from .recattn import RecAttn2d
from .recconv import RecConv2d

# model/recnext.py:365-407 and model/recattn.py:378-420
CONFIGS = {
    "recnext_m0": dict(family="m", embed_dim=(40, 80, 160, 320), depth=(2, 2, 9, 1)),
    "recnext_m1": dict(family="m", embed_dim=(48, 96, 192, 384), depth=(3, 3, 15, 2)),
    "recnext_m2": dict(family="m", embed_dim=(56, 112, 224, 448), depth=(3, 3, 15, 2)),
    "recnext_m3": dict(family="m", embed_dim=(64, 128, 256, 512), depth=(3, 3, 13, 2)),
    "recnext_m4": dict(family="m", embed_dim=(64, 128, 256, 512), depth=(5, 5, 25, 4), drop_path=0.2),
    "recnext_m5": dict(family="m", embed_dim=(80, 160, 320, 640), depth=(7, 7, 35, 2), drop_path=0.3),
    "recnext_a0": dict(family="a", embed_dim=(40, 80, 160, 320), depth=(2, 2, 9, 1)),
    "recnext_a1": dict(family="a", embed_dim=(48, 96, 192, 384), depth=(3, 3, 15, 2)),
    "recnext_a2": dict(family="a", embed_dim=(56, 112, 224, 448), depth=(3, 3, 15, 2)),
    "recnext_a3": dict(family="a", embed_dim=(64, 128, 256, 512), depth=(3, 3, 13, 2), mlp_ratio=1.875),
    "recnext_a4": dict(family="a", embed_dim=(64, 128, 256, 512), depth=(5, 5, 25, 4), mlp_ratio=1.875, drop_path=0.2),
    "recnext_a5": dict(family="a", embed_dim=(80, 160, 320, 640), depth=(7, 7, 35, 2), mlp_ratio=1.875, drop_path=0.3),
}


def default_token_mixer(family):
    if family == "m":   # model/recnext.py:152
        return lambda dim, stage: RecConv2d(dim, level=4 - stage, kernel_size=5)
    if family == "a":   # model/recattn.py:166
        return lambda dim, stage: RecAttn2d(dim, num_heads=2 ** (stage + 1), stage=stage)
    raise ValueError(f"unknown family {family!r}")


def channel_mlp(dim, hidden, act_layer):
    return nn.Sequential(ConvNorm(dim, int(hidden), kernel_size=1), act_layer(), ConvNorm(int(hidden), dim, kernel_size=1))


class RecNextStem(nn.Module):
    def __init__(self, in_channels, out_channels, act_layer=nn.GELU):
        super().__init__()
        self.stem = nn.Sequential(ConvNorm(in_channels, out_channels // 2, kernel_size=3, stride=2, padding=1), act_layer(),
                                  ConvNorm(out_channels // 2, out_channels, kernel_size=3, stride=2, padding=1))

    def forward(self, x):
        fused = self.__dict__.get("_fused_stem")
        if fused is not None and not self.training and fused.usable(self.stem, x):
            return fused(x)                             # one launch (use_fused_stem)
        if bnact.ATTR in self.__dict__:                 # use_fused_mixer_norms_train: ConvNorm -> GELU on BnGeluFn in a training forward
            mode = bnact.stem_ready(self, x)
            if mode is not None:
                return bnact.run_stem(self.stem, x, mode)
        return self.stem(x)


class MetaNeXtBlock(nn.Module):
    """x + drop_path(channel_mixer([norm](token_mixer(x)))); the M family has the BatchNorm, the A family does not."""

    def __init__(self, dim, mlp_ratio, act_layer, stage, drop_path, family, token_mixer):
        super().__init__()
        self.token_mixer = token_mixer(dim, stage)
        if family == "m":
            self.norm = nn.BatchNorm2d(dim)
        self.channel_mixer = channel_mlp(dim, dim * mlp_ratio, act_layer)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self._has_norm = family == "m"

    def forward(self, x):
        t = self.token_mixer(x)
        if self._has_norm:
            t = self.norm(t)
        fused = self.__dict__.get("_fused_mlp")
        if fused is not None and not self.training and fused.usable(self.channel_mixer, t, x):
            return fused(t, x)                          # x + channel_mixer(t) in one launch (use_fused_mlp)
        if bnact.ATTR in self.channel_mixer.__dict__:   # use_fused_mixer_norms_train: the mixer's two norms with their epilogues in a training forward
            mode = bnact.mixer_ready(self.channel_mixer, t)
            if mode is not None:
                return bnact.run_mixer(self.channel_mixer, t, x, self.drop_path, mode)
        return x + self.drop_path(self.channel_mixer(t))


class Downsample(nn.Module):
    def __init__(self, in_channels, mlp_ratio, act_layer):
        super().__init__()
        out_channels = in_channels * 2
        self.token_mixer = nn.Conv2d(in_channels, out_channels, kernel_size=7, padding=3, groups=in_channels, stride=2)
        self.norm = nn.BatchNorm2d(out_channels)
        self.channel_mixer = channel_mlp(out_channels, out_channels * mlp_ratio, act_layer)
        object.__setattr__(self, "_hip", None)          # set by use_hip_downsample; never a registered child (state_dict keys stay)

    def _hip_path(self):
        """The HIP reroute if it still wraps THIS module's current children.  A child replaced after use_hip_downsample
        (SyncBatchNorm.convert_sync_batchnorm, a fusion pass, `m.norm = ...`) must be followed: the old module's parameters
        are in neither state_dict nor the optimizer any more.  Whole-model pickles from before the reroute existed have no attribute."""
        hip = self.__dict__.get("_hip")
        if hip is not None and (hip.token_mixer is not self.token_mixer or hip.norm is not self.norm):
            hip = None
            if isinstance(self.token_mixer, nn.Conv2d) and type(self.norm) is nn.BatchNorm2d:
                from .dwconv import DownsampleDwConv
                try:
                    hip = DownsampleDwConv(self.token_mixer, self.norm)
                except ValueError:                       # not the depthwise C -> 2C conv any more: the PyTorch operators
                    hip = None
            object.__setattr__(self, "_hip", hip)
        return hip

    def forward(self, x):
        hip = self._hip_path()
        x = hip(x) if hip is not None else self.norm(self.token_mixer(x))
        fused = self.__dict__.get("_fused_mlp")
        if fused is not None and not self.training and fused.usable(self.channel_mixer, x, x):
            return fused(x, x)
        if bnact.ATTR in self.channel_mixer.__dict__:
            mode = bnact.mixer_ready(self.channel_mixer, x)
            if mode is not None:
                return bnact.run_mixer(self.channel_mixer, x, x, None, mode)
        return x + self.channel_mixer(x)


class RecNextClassifier(nn.Module):
    def __init__(self, dim, num_classes, distillation=False, drop=0.0):
        super().__init__()
        self.head_drop = nn.Dropout(drop)
        self.head = NormLinear(dim, num_classes) if num_classes > 0 else nn.Identity()
        self.head_dist = NormLinear(dim, num_classes) if num_classes > 0 else nn.Identity()
        self.distillation = distillation
        self.num_classes = num_classes

    def forward(self, x):
        x = self.head_drop(x)
        a, b = self.head(x), self.head_dist(x)
        if self.training and self.distillation:
            return a, b
        return (a + b) / 2

    @torch.no_grad()
    def fuse(self):
        if self.num_classes <= 0:
            return nn.Identity()
        a, b = self.head.fuse(), self.head_dist.fuse()
        a.weight.copy_((a.weight + b.weight) / 2)
        a.bias.copy_((a.bias + b.bias) / 2)
        return a


class RecNextStage(nn.Module):
    def __init__(self, in_channels, out_channels, depth, mlp_ratio, act_layer, downsample, stage, drop_path, family, token_mixer):
        super().__init__()
        self.downsample = Downsample(in_channels, mlp_ratio, act_layer) if downsample else nn.Identity()
        self.blocks = nn.Sequential(*[MetaNeXtBlock(out_channels, mlp_ratio, act_layer, stage, drop_path, family, token_mixer)
                                      for _ in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class RecNext(nn.Module):
    def __init__(self, family="m", in_chans=3, embed_dim=(48,), depth=(2,), mlp_ratio=2, global_pool="avg", num_classes=1000,
                 act_layer=nn.GELU, distillation=False, drop_rate=0.0, drop_path=0.0, token_mixer=None):
        super().__init__()
        token_mixer = token_mixer or default_token_mixer(family)
        self.family = family
        self.global_pool = global_pool
        self.embed_dim = tuple(embed_dim)
        self.num_classes = num_classes
        self.stem = RecNextStem(in_chans, embed_dim[0], act_layer)
        stages, prev = [], embed_dim[0]
        for i, (dim, d) in enumerate(zip(embed_dim, depth)):
            stages.append(RecNextStage(prev, dim, d, mlp_ratio, act_layer, downsample=i != 0, stage=i, drop_path=drop_path,
                                       family=family, token_mixer=token_mixer))
            prev = dim
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
    """``timm.create_model`` stand-in for the twelve registered names (model/recnext.py:365-407, model/recattn.py:378-420) and the LSNet-style
    recnext_t / _s / _b (lsnet/model/recattn.py:441-466, built by recnext_amd.lsmodels; ``token_mixer(dim, num_heads, stage)`` there) and their
    share-channel siblings recnext_t_share_channel / _s_ / _b_ (lsnet/model/recattn_share_channel.py:461-485, built by recnext_amd.lsshare)."""
    if name not in CONFIGS:
        from . import lsmodels
        if name in lsmodels.LS_CONFIGS:
            return lsmodels.create_model(name, distillation=distillation, token_mixer=token_mixer, **overrides)
        from . import lsshare
        if name in lsshare.SHARE_CONFIGS:
            return lsshare.create_model(name, distillation=distillation, token_mixer=token_mixer, **overrides)
    cfg = dict(CONFIGS[name])
    if distillation:
        cfg["drop_path"] = 0.0                      # drop_path applies to the non-distilled recipe only
    cfg.update(overrides)
    return RecNext(distillation=distillation, token_mixer=token_mixer, **cfg)


def _mlp_hosts():
    """The module types whose ``channel_mixer`` the pointwise / fused-MLP passes rewrite: the M / A families' and the T / S / B family's blocks and Downsamples."""
    from . import lsmodels
    return (MetaNeXtBlock, Downsample, lsmodels.MetaNeXtBlock, lsmodels.Downsample)


def replace_batchnorm(net):
    """utils.replace_batchnorm (utils.py:227-234): swap every child that knows how to ``fuse`` itself, recursively.

    Plain ``nn.BatchNorm2d`` children (MetaNeXtBlock.norm, Downsample.norm) have no ``fuse`` and stay.
    """
    for name, child in list(net.named_children()):
        if hasattr(child, "fuse"):
            fused = child.fuse()
            setattr(net, name, fused)
            replace_batchnorm(fused)
        else:
            replace_batchnorm(child)
    return net


@torch.no_grad()
def fold_token_mixer_norms(net):
    """Inference-only: absorb each MetaNeXtBlock's eval-mode ``norm`` (a per-channel affine that
    ``replace_batchnorm`` leaves in place, utils.py:227-234) into its HIP token mixer's final conv.

    x + mlp(norm(mixer(x)))  ==  x + mlp(mixer'(x))  with  convs[level]' = scale*convs[level] + shift.
    Returns the number of BatchNorm layers removed (21 for RecNeXt-M3).  SURVEY.md section 8f row 2.
    """
    n = 0
    for m in net.modules():
        if isinstance(m, MetaNeXtBlock) and m._has_norm and isinstance(m.norm, nn.BatchNorm2d) \
                and isinstance(m.token_mixer, RecConv2d):
            if m.norm.training:
                raise RuntimeError("fold_token_mixer_norms needs eval mode (running statistics)")
            bn = m.norm
            scale = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
            shift = bn.bias.float() - scale * bn.running_mean.float()
            m.token_mixer.fold_output_affine(scale, shift)
            m.norm = nn.Identity()
            m._has_norm = False
            n += 1
    return n


@torch.no_grad()
def use_hip_downsample(net):
    """Run each Downsample's strided conv on HIP.  M / A families: the depthwise 7x7 stride-2 conv (C -> 2C), in eval
    mode fused with the BatchNorm after it into one kernel, in a training step with a HIP backward and the norm on batch statistics.  T / S / B
    families (``lsmodels.Downsample``, the share-channel models' too): the grouped 5x5 stride-2 ConvNorm as one launch (``ops.grouped_conv2d``) in an
    inference forward; training and forwards that need a gradient keep the library conv.
    ``token_mixer`` and ``norm`` remain the Downsample's direct children (same state_dict keys as the reference, so checkpoints
    load and save unchanged in either order); only the forward is rerouted.  Returns the number of layers rerouted."""
    from . import lsmodels
    from .dwconv import DownsampleDwConv
    n = 0
    for m in net.modules():
        if isinstance(m, Downsample) and m._hip is None and isinstance(m.token_mixer, nn.Conv2d) and isinstance(m.norm, nn.BatchNorm2d):
            object.__setattr__(m, "_hip", DownsampleDwConv(m.token_mixer, m.norm))
            n += 1
        elif isinstance(m, lsmodels.Downsample) and not m.__dict__.get("_hip") and m._conv() is not None:
            m._hip = True
            n += 1
    return n


def use_hip_batchnorm(net, all_shapes=False):
    """Run every plain ``nn.BatchNorm2d`` of ``net`` (a model of ``models``, ``lsmodels`` or ``lsshare``) on the HIP BatchNorm in a training step, and in
    eval mode where a gradient flows (frozen statistics): each module whose type is exactly ``nn.BatchNorm2d`` becomes a ``batchnorm.HipBatchNorm2d``
    by a change of class in place.  The module object, its Parameters and buffers stay the very same objects, so state_dict keys, strict loads in
    either order, optimizers, packs keyed by parameter address, ``Downsample._hip_path``'s identity check and ``GraphedInference`` stay valid, and
    ``SyncBatchNorm.convert_sync_batchnorm`` still converts the modules.  A call takes the HIP path only for the shapes the routing rule keeps
    (``batchnorm.batch_norm_routed``: those measured faster than the library's BatchNorm); ``all_shapes`` routes every shape the kernels take.
    Opt-in: nothing calls it by default.  Returns the number of modules changed (0 on a second call)."""
    from .batchnorm import HipBatchNorm2d
    n = 0
    for m in net.modules():
        if type(m) is nn.BatchNorm2d:
            m.__class__ = HipBatchNorm2d
            if all_shapes:
                m.hip_all_shapes = True
            n += 1
    return n


def _mark(module, attr, all_shapes):
    """Mark `module` for one of the ``use_fused_*_train`` operators: the plain attribute `attr` = "all" | "measured".  -> 1 if newly marked, else 0.

    What the three calls share.  The mark is a plain attribute and nothing else: state_dict keys, Parameters, buffers and module objects are
    untouched, strict loads work in either order.  A marked module takes its operator in a call when the tensor is a GPU tensor of float32 /
    bfloat16 / float16 with more than one (output) value a channel, every norm it takes over is exactly ``nn.BatchNorm2d`` or ``HipBatchNorm2d`` in
    training mode, affine with float32 parameters, float32 running buffers (or none) and a float momentum (``batchnorm.norm_fusable``), and the
    shape is one the operator's routing rule keeps (``all_shapes`` routes every shape the kernels take); each such norm's ``num_batches_tracked`` is
    then bumped by one (``batchnorm.bump``).  Everything else -- eval-mode or frozen norms, SyncBatchNorm, ``momentum=None``, 16-bit parameters, a
    folded ``nn.Conv2d``, CPU -- keeps the operator chain, unchanged.  Opt-in: nothing calls them by default; each returns the number of modules
    newly marked (0 on a second call)."""
    new = 0 if module.__dict__.get(attr) else 1
    setattr(module, attr, "all" if all_shapes else "measured")
    return new


def use_fused_rep_train(net, all_shapes=False):
    """Run every unfused ``RepVGGDW`` of ``net`` (the T / S / B models of ``lsmodels`` and the share-channel models of ``lsshare``) as one HIP operator
    in a training step: ``ops.RepDwFn`` (``recnext_amd/repdw.py``), three launches forward and at most four backward in place of the operator chain of
    ``lsmodels._rep_train``.  The mark, what a marked module asks of a call and what keeps the chain: ``_mark``.  Particular to this one: both convs
    have float32 weights and biases, both norms have running buffers or neither has, and the rule is ``repdw.repdw_train_routed``."""
    from . import lsmodels
    return sum(_mark(m, "_fused_rep_train", all_shapes) for m in net.modules() if isinstance(m, lsmodels.RepVGGDW))


def use_fused_conv_norm_train(net, all_shapes=False):
    """Run the depthwise ``ConvNorm``s of every slice mixer of ``net`` as one HIP operator each in a training step: ``down[0]``, ``pe`` and ``conv`` of every
    ``RecAttn2d`` (the M / A families) and ``LsRecAttn2d`` (T / S / B) and ``pe`` of every ``LinearAttention3`` -- the modules
    ``recattn._conv_norm_train`` / ``_upadd_conv_norm_train`` are called with by the mixers -- run ``ops.DwConvBnFn`` (``recnext_amd/dwbn.py``), three
    launches forward and at most five backward in place of the conv's Function followed by the module's BatchNorm.  (``RepVGGDW.lk`` has its own
    operator: ``use_fused_rep_train``.)  The mark, what a marked module asks of a call and what keeps the chain: ``_mark``.  Particular to this one: the
    conv's weight (and bias, if it has one) is float32, the resize mode of the up-add form is ``"nearest"`` (bilinear keeps the chain), and the rule is
    ``dwbn.dwconv_bn_train_routed``, on the output rows."""
    from . import lsmodels
    from .layers import ConvNorm
    from .recattn import LinearAttention, RecAttn2d
    n = 0
    for m in net.modules():
        if isinstance(m, RecAttn2d):
            hosts = (m.down[0], m.conv)
        elif isinstance(m, (LinearAttention, lsmodels.LinearAttention3)):
            hosts = (m.pe,)
        else:
            continue
        for cn in hosts:
            if isinstance(cn, ConvNorm):
                n += _mark(cn, "_fused_conv_norm_train", all_shapes)
    return n


def use_fused_mixer_norms_train(net, all_shapes=False):
    """Run the two BatchNorms of every channel mixer of ``net`` with what follows them as one HIP operator each in a training step: a marked mixer
    ``[ConvNorm, GELU, ConvNorm]`` runs ``seq[0].conv(t) -> ops.BnGeluFn -> seq[2].conv(z) -> ops.BnAddFn(u2, r, mask)`` (``recnext_amd/bnact.py``):
    ``GELU(BN(u1))`` without a stored ``BN(u1)``, and ``r + drop_path(BN(u2))`` with the DropPath mask drawn as ``DropPath.forward`` draws it (the same
    random stream, the same values), three launches forward and three backward each in place of the BatchNorm, the GELU, the mask multiply and the add.
    A marked stem runs each ``ConvNorm -> exact GELU`` pair on ``ops.BnGeluFn``; a ``ConvNorm`` followed by ``nn.Identity`` keeps the chain.  Marked:
    the ``channel_mixer`` of every ``MetaNeXtBlock`` / ``Downsample`` of this module and of ``lsmodels`` (the share-channel models' blocks among them) and
    both ``RecNextStem``s.  The mark, what a marked module asks of a call and what keeps the chain: ``_mark``.  Particular to this one: the attribute is
    set on the ``nn.Sequential`` (on the stem module) and holds the very layers besides the mode (``bnact.mark``), the mixer must still be ``[ConvNorm,
    exact GELU, ConvNorm]`` of those layers, unhooked, each norm decides for itself by ``bnact.bn_act_routed``, and the inference-only ``_fused_mlp``
    path comes first."""
    from . import lsmodels
    n = 0
    for m in net.modules():
        if isinstance(m, _mlp_hosts()) and isinstance(m.channel_mixer, nn.Sequential):
            n += bnact.mark(m.channel_mixer, m.channel_mixer, all_shapes)
        elif isinstance(m, (RecNextStem, lsmodels.RecNextStem)) and isinstance(m.stem, nn.Sequential):
            n += bnact.mark(m, m.stem, all_shapes)
    return n


def use_linear_pointwise(net):
    """Inference-only plumbing: evaluate the (BN-folded) 1x1 convs of every channel mixer through the GEMM library
    (bias in the epilogue) instead of the conv library (bias as a separate kernel).  Returns the number replaced."""
    from .layers import PointwiseLinear
    n = 0
    for m in net.modules():
        if isinstance(m, _mlp_hosts()):
            seq = m.channel_mixer
            for i, sub in enumerate(seq):
                if isinstance(sub, nn.Conv2d) and sub.kernel_size == (1, 1) and sub.groups == 1 and sub.bias is not None:
                    seq[i] = PointwiseLinear(sub)
                    n += 1
    return n


def use_fused_stem(net):
    """Inference-only, after ``replace_batchnorm``: evaluate RecNextStem ([3x3 stride-2 conv + bias, exact GELU, 3x3 stride-2 conv + bias]) as ONE HIP launch where
    rcx_stem_fwd has a kernel (bf16 on a GPU; decided per call) -- the 112 x 112 intermediate never reaches memory -- and the T / S / B ``lsmodels.RecNextStem``
    ([conv, GELU, conv, GELU, conv, GELU | Identity]) as the two launches of rcx_stem3_fwd likewise.  The convs, their parameters and the state_dict
    are untouched.  Returns the number of stems given the fused path (0 or 1)."""
    from .layers import FusedStem, FusedStem3, _is_exact_gelu
    from .lsmodels import RecNextStem as LsStem

    def stem_conv(m):
        return isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (2, 2) and m.padding == (1, 1) and m.groups == 1 and m.dilation == (1, 1)

    n = 0
    for m in net.modules():
        if not isinstance(m, (RecNextStem, LsStem)) or m.__dict__.get("_fused_stem") is not None:
            continue
        seq = m.stem
        if isinstance(m, RecNextStem):
            if len(seq) == 3 and stem_conv(seq[0]) and stem_conv(seq[2]) and _is_exact_gelu(seq[1]) and seq[0].in_channels == 3:
                object.__setattr__(m, "_fused_stem", FusedStem(seq[0], seq[2]))
                n += 1
        elif len(seq) == 6 and all(stem_conv(seq[i]) and seq[i].bias is not None for i in (0, 2, 4)) and _is_exact_gelu(seq[1]) and _is_exact_gelu(seq[3]) \
                and (_is_exact_gelu(seq[5]) or type(seq[5]) is nn.Identity) and seq[0].in_channels == 3:
            object.__setattr__(m, "_fused_stem", FusedStem3(seq[0], seq[2], seq[4], _is_exact_gelu(seq[5])))
            n += 1
    return n


def use_fused_head(net, all_shapes=False):
    """Inference-only: evaluate ``forward_head`` -- ``head(head_drop(x.mean((2, 3))))`` -- of a ``RecNext`` (this module's, ``lsmodels``' and the
    share-channel models built on it) as ONE HIP launch (``ops.pool_head``, rcx_pool_head_fwd: float32 arithmetic, one rounding at the store) where the
    call allows it, decided per call (``head.FusedHead.usable``): eval mode, ``global_pool == "avg"``, a dense channels_last GPU tensor of float32 /
    bfloat16 / float16, no gradient wanted, ``net.head`` still the module it was here -- the ``nn.Linear`` ``replace_batchnorm`` leaves (its weight taken
    as it lies), an eval-mode unfused ``RecNextClassifier`` (folded and averaged in float32 at pack time) or the ``nn.Identity`` of ``num_classes=0``
    (``ops.global_pool``) -- and a shape the routing rule keeps (``head.pool_head_routed``; ``all_shapes`` routes every shape the kernel takes).
    Everything else -- training, distillation in train mode, a CPU tensor, NCHW strides, a replaced head -- is the path as it was.  The call sets the
    plain attribute ``_fused_head`` and nothing else: keys, Parameters and buffers are untouched.  Opt-in: nothing calls it by default.  Returns 1, or
    0 when ``net`` is no such model or already has the helper for the head it has now (a helper for a head since replaced, by ``replace_batchnorm`` for one,
    is renewed)."""
    from . import lsmodels
    from .head import FusedHead
    if not isinstance(net, (RecNext, lsmodels.RecNext)):
        return 0
    have = net.__dict__.get("_fused_head")
    if have is not None and have.head is net.head:
        return 0
    object.__setattr__(net, "_fused_head", FusedHead(net, all_shapes=all_shapes))
    return 1


def use_fused_mlp(net):
    """Inference-only, after ``use_linear_pointwise``: evaluate ``x + channel_mixer(t)`` of every MetaNeXtBlock / Downsample whose mixer is
    [1x1 conv, exact GELU, 1x1 conv] as ONE HIP launch where rcx_channel_mlp_fwd has a kernel (bf16; the 56 x 56 and 28 x 28 stages, where the two GEMMs
    are memory-bound and the hidden tensor's round trips are most of their time) -- other blocks, dtypes and devices keep the GEMM library, decided per
    call.  The layers, their parameters and the state_dict are untouched.  Returns the number of blocks given the fused path."""
    from .layers import FusedChannelMlp, PointwiseLinear
    n = 0
    for m in net.modules():
        if isinstance(m, _mlp_hosts()) and m.__dict__.get("_fused_mlp") is None:
            seq = m.channel_mixer
            if len(seq) == 3 and isinstance(seq[0], PointwiseLinear) and isinstance(seq[2], PointwiseLinear) and isinstance(seq[1], nn.GELU) \
                    and getattr(seq[1], "approximate", "none") == "none":            # (drop_path is the identity in eval mode, the only mode the fused path runs in)
                object.__setattr__(m, "_fused_mlp", FusedChannelMlp(seq[0], seq[2]))
                n += 1
    return n


def padded_hidden_width(hidden, max_growth=0.125):
    """The hidden width the channel mixers' GEMMs run at: the next multiple of 64 (else of 16) when that adds at most ``max_growth``, else unchanged."""
    for mult in (64, 16):
        hp = -(-hidden // mult) * mult
        if hp != hidden and hp <= hidden * (1 + max_growth):
            return hp
    return hidden


def pad_mlp_hidden(net):
    """Inference-only plumbing, after ``use_linear_pointwise``: run the two GEMMs of a channel mixer at a zero-padded hidden width (RecNeXt-A's
    1.875 x dim -- 120 / 240 / 480 -- become 128 / 256 / 512).  The same function: a padded hidden channel is act(0 + 0) = 0 and meets zero weights
    (checked: the activation must map 0 to 0).  Parameters and ``state_dict`` are untouched (``PointwiseLinear.pad``).  Returns the mixers changed."""
    from .layers import PointwiseLinear
    n = 0
    for m in net.modules():
        if isinstance(m, _mlp_hosts()):
            seq = m.channel_mixer
            if len(seq) != 3 or not isinstance(seq[0], PointwiseLinear) or not isinstance(seq[2], PointwiseLinear):
                continue
            with torch.no_grad():
                if float(seq[1](torch.zeros(1)).abs().max()) != 0.0:
                    continue
            hp = padded_hidden_width(seq[0].out_channels)
            if hp != seq[0].out_padded or hp != seq[2].in_padded:
                seq[0].pad(out_to=hp)
                seq[2].pad(in_to=hp)
                n += hp != seq[0].out_channels
    return n


def token_mixer_shapes(name, resolution=224):
    """[(C, H, W, level|None, count)] of every token mixer call in one forward pass (SURVEY 8 model tables)."""
    cfg = CONFIGS[name]
    out = []
    side = resolution // 4
    for s, (dim, d) in enumerate(zip(cfg["embed_dim"], cfg["depth"])):
        out.append((dim, side, side, 4 - s if cfg["family"] == "m" else None, d))
        side = (side + 1) // 2 if s < 3 else side      # Downsample: k7 s2 p3 -> ceil(side/2)
    return out


def token_mixer_algorithmic_bytes(name, resolution=224, elem_bytes=2, k=5):
    """Compulsory traffic of all RecConv2d blocks for ONE image: 2*C*H*W*b + (level+2)*C*k*k*b per block."""
    total = 0
    for (c, h, w, level, count) in token_mixer_shapes(name, resolution):
        if level is None:
            raise ValueError("defined for the M family")
        total += count * (2 * c * h * w * elem_bytes + (level + 2) * c * k * k * elem_bytes)
    return total
