"""PyTorch-operator restatement of the share-channel RecNeXt-T / S / B (lsnet/model/recattn_share_channel.py:37-124, :281-326), for the tests.

The slice mixers are tests/ls_eager.py's with one head each; the share stage is restated here: a block with a slice mixer computes
``r = RepVGGDW(x)``, ``x1 = mixer(r[:, :s])``, ``t = cat(x1, r[:, s:])`` and remembers x1; a share block computes ``t = r + cat(the remembered x1s)``
and forgets them.  ``models.create_model("recnext_t_share_channel", token_mixer=eager_share_token_mixer)`` builds a model whose every token half
runs on these operators (a token_mixer override keeps recnext_amd.lsshare's share blocks on library operators too); ``share_stage_forward`` and
``share_token_half`` run a stage or one share block of ANY model of the family on them, in any dtype (float64 for the training tests).
Pinned to the reference by tests/golden/ls_share_*.npz (tests/test_ls_share_cpu.py).
"""
import torch

from tests.ls_eager import EagerLinearAttention3, EagerRecAttn2d


def eager_share_token_mixer(dim, num_heads, stage):
    """The slice-mixer factory of lsshare.create_model(token_mixer=...): one head everywhere, LinearAttention3 from stage 2 on."""
    if stage >= 2:
        return EagerLinearAttention3(dim, 2)                # its constructor halves the count: the module's own num_heads is 1
    return EagerRecAttn2d(dim, 1, stage=stage)


def share_token_half(block, x, x1s):
    """(r, t) of a share block: r = rep_mixer(x), t = r + the remembered slice-mixer outputs side by side."""
    r = block.rep_mixer(x)
    return r, r + torch.cat(list(x1s), dim=1)


def mixer_token_half(block, x):
    """(r, t, x1) of a block with a slice mixer built by eager_share_token_mixer."""
    attn = block.token_mixer.attn
    if not isinstance(attn, (EagerRecAttn2d, EagerLinearAttention3)):
        raise TypeError("mixer_token_half needs a block built with token_mixer=eager_share_token_mixer")
    r = block.rep_mixer(x)
    s = block.token_mixer.split_idx
    x1 = attn(r[:, :s])
    return r, torch.cat([x1, r[:, s:]], dim=1), x1


def share_stage_forward(stage, x, halves=None):
    """The forward of an lsshare.RecNextStage (built with the eager mixers) on the operator chain; `halves`, a list, receives every block's (r, t)."""
    x = stage.downsample(x)
    remembered = []
    for block in stage.blocks:
        if block.is_share_block:
            r, t = share_token_half(block, x, remembered)
            remembered = []
        else:
            r, t, x1 = mixer_token_half(block, x)
            if stage.is_share_stage:
                remembered.append(x1)
        if halves is not None:
            halves.append((r, t))
        x = r + block.drop_path(block.channel_mixer(t))
    return x
