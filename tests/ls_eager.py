"""PyTorch-operator restatement of the LSNet-style RecNeXt-T / S / B slice mixers (lsnet/model/recattn.py:37-127), for the tests.

Same module and parameter names as the reference and as recnext_amd.lsmodels, so one state_dict loads into either.  Plug it into a model with
``models.create_model("recnext_t", token_mixer=eager_token_mixer)``: the block then computes r = RepVGGDW(x) and t = cat(mixer(r[:, :C/4]), r[:, C/4:])
with library operators.  Pinned to the reference by tests/golden/ls_*.npz (tests/test_lsnet_cpu.py).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from recnext_amd.lsmodels import ConvNorm


def _attend(q, k, v, s):
    """q (b, heads, dq, n), k like q, v (b, heads, dv, n) -> (b, heads, n, dv): q (k^T v) s^2 / (q . mean(k) + 1e-6) (:47-52)."""
    q_t = q.transpose(-1, -2)
    kv = (k * s) @ (v.transpose(-1, -2) * s)
    return q_t @ kv / (q_t @ k.mean(dim=-1, keepdim=True) + 1e-6)


class EagerLinearAttention(nn.Module):
    """LinearAttention1 (:37-58); LinearAttention2 (:61-86) is the same function."""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.qk = ConvNorm(dim, dim * 2, kernel_size=1, groups=2)
        self.pe = ConvNorm(dim, dim, kernel_size=3, padding=1, groups=dim)

    def forward(self, x):
        b, c, h, w = x.shape
        n = h * w
        qk = F.elu(self.qk(x)) + 1.0
        q, k = qk.view(b, 2, self.num_heads, self.head_dim, n).unbind(dim=1)
        o = _attend(q, k, x.view(b, self.num_heads, self.head_dim, n), n ** -0.5)
        return o.transpose(-1, -2).reshape(b, c, h, w) + self.pe(x)


class EagerRecAttn2d(nn.Module):
    """RecAttn2d (:115-127): conv(x + nearest(LA(down(x))))."""

    def __init__(self, dim, num_heads, kernel_size=5, stage=1, mode="nearest"):
        super().__init__()
        self.mode = mode
        self.down = nn.Sequential(ConvNorm(dim, dim, kernel_size=kernel_size, padding=kernel_size // 2, stride=2, groups=dim),
                                  EagerLinearAttention(dim, num_heads))
        self.conv = ConvNorm(dim, dim, kernel_size=kernel_size, padding=kernel_size // 2, groups=dim)

    def forward(self, x):
        return self.conv(x + F.interpolate(self.down(x), size=x.shape[2:], mode=self.mode))


class EagerLinearAttention3(nn.Module):
    """LinearAttention3 (:89-112): a full 1x1 qk, q and k of dim / 2 channels, v the input."""

    def __init__(self, dim, num_heads, **kwargs):
        super().__init__()
        self.num_heads = num_heads // 2
        self.head_dim = dim // self.num_heads // 2
        self.qk = ConvNorm(dim, dim, kernel_size=1, groups=1)
        self.pe = ConvNorm(dim, dim, kernel_size=3, padding=1, groups=dim)

    def forward(self, x):
        b, c, h, w = x.shape
        n = h * w
        qk = F.elu(self.qk(x)) + 1.0
        q, k = qk.view(b, 2, self.num_heads, self.head_dim, n).unbind(dim=1)
        o = _attend(q, k, x.view(b, self.num_heads, -1, n), n ** -0.5)
        return o.transpose(-1, -2).reshape(b, c, h, w) + self.pe(x)


def eager_token_mixer(dim, num_heads, stage):
    """The slice-mixer factory of lsmodels.create_model(token_mixer=...): the operator chain in place of the HIP token half."""
    if stage >= 3:
        return EagerLinearAttention3(dim, num_heads)
    return EagerRecAttn2d(dim, num_heads, stage=stage)


def token_half(block, x):
    """(r, t) of an lsmodels.MetaNeXtBlock on the operator chain, whatever its slice mixer: r = rep_mixer(x), t = cat(mixer(r_s), r[:, s:])."""
    r = block.rep_mixer(x)
    s = block.token_mixer.split_idx
    attn = block.token_mixer.attn
    if not isinstance(attn, (EagerRecAttn2d, EagerLinearAttention3)):
        raise TypeError("token_half needs a block built with token_mixer=eager_token_mixer")
    return r, torch.cat([attn(r[:, :s]), r[:, s:]], dim=1)
