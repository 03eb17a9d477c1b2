#!/usr/bin/env python3
"""Generate the share-channel RecNeXt-T / S / B fixtures (tests/golden/ls_share_*) by IMPORTING the reference (build container only).

    python tests/golden/make_golden_ls_share.py --reference <checkout of the reference>

Runs lsnet/model/recattn_share_channel.py on torch CPU under make_golden.py's timm shim and stores data only:
  ls_share_block_<H>x<W>_c<C>.npz   one share block's token half: x and the four slice-mixer outputs x1 (bf16-representable, stored as bf16 bits), the
                                    block's rep_mixer parameters with non-trivial BN statistics, r = rep_mixer(x) and t = r + cat(x1s) in float32;
  ls_share_la3_14x14_c<C>.npz       one stage-2 mixer block's token half (LinearAttention3 on a 14 x 14 plane), in make_golden_ls.py's ls_block_* format;
  ls_share_tiny_model.npz           a tiny RecNext of this family (embed_dim (32, 64, 96, 128), depth (1, 1, 2, 6): one share block and a trailing
  ls_share_tiny_model_stage3.npz    mixer block nobody reads; 128 x 128 input, 10 classes): bf16-representable parameters and input as bf16 bits (the
                                    share stage's in the second file), float32 logits before and after fuse();
  ls_share_models.json              the unfused and fused state_dict key lists and parameter counts of the three registered names.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
from make_golden_ls import bf16_bits  # noqa: E402

# (name, B, C, H, W, mlp_ratio, seed)
SHARE_BLOCKS = [("4x4_c512", 2, 512, 4, 4, 1.5, 60), ("3x5_c16", 2, 16, 3, 5, 1.5, 61)]
# (name, C, H, mlp_ratio, seed): T's and S / B's stage 2
LA3_BLOCKS = [("14x14_c256", 256, 14, 2, 62), ("14x14_c384", 384, 14, 2, 63)]
NAMES = ("recnext_t_share_channel", "recnext_s_share_channel", "recnext_b_share_channel")


def gen_share_blocks(refs, out):
    for (name, b, c, h, w, ratio, seed) in SHARE_BLOCKS:
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        blk = refs.MetaNeXtBlock(c, ratio, stage=3, block=4, split_rate=4, is_share_stage=True).eval()
        assert blk.is_share_block
        make_golden.randomize_bn(blk, gen)
        x = make_golden.bf16_round(torch.randn(b, c, h, w, generator=gen))
        x1s = [make_golden.bf16_round(torch.randn(b, c // 4, h, w, generator=gen)) for _ in range(4)]
        with torch.no_grad():
            r = blk.rep_mixer(x)
            t = blk.token_mixer(r, x1s)
        rec = {"x_bf16": bf16_bits(x), "r": make_golden.np32(r), "t": make_golden.np32(t),
               "meta": np.array(json.dumps(dict(B=b, C=c, H=h, W=w, mlp_ratio=ratio, split=c // 4, seed=seed)))}
        rec.update({f"x1_{j}_bf16": bf16_bits(s) for j, s in enumerate(x1s)})
        rec.update({"sd::" + k: make_golden.np32(v) for k, v in blk.state_dict().items() if v.dtype.is_floating_point and k.startswith("rep_mixer.")})
        np.savez(os.path.join(out, f"ls_share_block_{name}.npz"), **rec)
        print("ls share block", name, tuple(t.shape))


def gen_la3_blocks(refs, out):
    for (name, c, h, ratio, seed) in LA3_BLOCKS:
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        blk = refs.MetaNeXtBlock(c, ratio, stage=2, block=0, split_rate=4, is_share_stage=False).eval()
        make_golden.randomize_bn(blk, gen)
        x = make_golden.bf16_round(torch.randn(1, c, h, h, generator=gen))
        with torch.no_grad():
            r = blk.rep_mixer(x)
            s = blk.token_mixer.part
            t_s = blk.token_mixer.attn(r[:, :s])
        rec = {"x_bf16": bf16_bits(x), "r": make_golden.np32(r), "t_s": make_golden.np32(t_s),
               "meta": np.array(json.dumps(dict(C=c, stage=2, H=h, W=h, num_heads=1, mlp_ratio=ratio, split=s, seed=seed)))}
        rec.update({"sd::" + k: make_golden.np32(v) for k, v in blk.state_dict().items()
                    if v.dtype.is_floating_point and not k.startswith("channel_mixer.")})
        np.savez(os.path.join(out, f"ls_share_la3_{name}.npz"), **rec)
        print("ls share la3 block", name, tuple(t_s.shape))


def gen_tiny(refs, out):
    torch.manual_seed(64)
    gen = torch.Generator().manual_seed(64)
    net = refs.RecNext(embed_dim=(32, 64, 96, 128), depth=(1, 1, 2, 6), mlp_ratios=(2, 2, 2, 1.5), split_rates=(4, 4, 4, 4), share_stage=3,
                       num_classes=10).eval()
    assert [b.is_share_block for b in net.stages[3].blocks] == [False] * 4 + [True, False]
    make_golden.randomize_bn(net, gen)
    for v in net.state_dict().values():                       # bf16-representable parameters and statistics: stored as bf16 bits, half the bytes
        if v.dtype.is_floating_point:
            v.copy_(make_golden.bf16_round(v))
    x = make_golden.bf16_round(torch.randn(2, 3, 128, 128, generator=gen))
    with torch.no_grad():
        logits = net(x)
        sd = {k: bf16_bits(v) for k, v in net.state_dict().items() if v.dtype.is_floating_point}
        net.fuse()
        logits_fused = net(x)
    # two files, each below the size limit of a committed file: the share stage's parameters apart from the rest
    rec = {"x_bf16": bf16_bits(x), "logits": make_golden.np32(logits), "logits_fused": make_golden.np32(logits_fused)}
    rec.update({"sd_bf16::" + k: v for k, v in sd.items() if not k.startswith("stages.3.")})
    np.savez(os.path.join(out, "ls_share_tiny_model.npz"), **rec)
    np.savez(os.path.join(out, "ls_share_tiny_model_stage3.npz"), **{"sd_bf16::" + k: v for k, v in sd.items() if k.startswith("stages.3.")})
    print("ls share tiny model", make_golden.np32(logits)[0, :3], f"fuse drift={float((logits - logits_fused).abs().max()):.2e}")


def gen_models(registry, out):
    rec = {}
    for name in NAMES:
        torch.manual_seed(0)
        net = registry[name]().eval()
        keys = list(net.state_dict().keys())
        params = sum(p.numel() for p in net.parameters())
        net.fuse()
        rec[name] = dict(keys=keys, params=params, fused_keys=list(net.state_dict().keys()), fused_params=sum(p.numel() for p in net.parameters()))
        print(name, params, rec[name]["fused_params"])
    with open(os.path.join(out, "ls_share_models.json"), "w") as f:
        json.dump(rec, f, indent=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.set_num_threads(4)
    registry = make_golden.install_timm_shim()
    refs = make_golden.load_by_path("ref_lsnet_recattn_share_channel", os.path.join(args.reference, "lsnet", "model", "recattn_share_channel.py"))
    gen_share_blocks(refs, args.out)
    gen_la3_blocks(refs, args.out)
    gen_tiny(refs, args.out)
    gen_models(registry, args.out)


if __name__ == "__main__":
    main()
