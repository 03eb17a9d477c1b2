#!/usr/bin/env python3
"""Generate the LSNet-style RecNeXt-T / S / B fixtures (tests/golden/ls_*) by IMPORTING the reference (build container only).

    python tests/golden/make_golden_ls.py [--reference /root/reference]

Runs lsnet/model/recattn.py on torch CPU under make_golden.py's timm shim and stores data only:
  ls_block_<H>x<W>_c<C>.npz  one MetaNeXtBlock token half per mixer shape of T / S / B at 224 (x, the block's rep_mixer / token_mixer parameters with
                             non-trivial BN statistics, r = rep_mixer(x), t_s = the slice mixer's output).  x is bf16-representable and is stored as
                             bf16 bits, so the float32 outputs are also the float32 reference on bf16-rounded input;
  ls_tiny_model.npz          a tiny RecNext (embed_dim (16, 32, 48, 64), depth (1, 1, 1, 1), 64 x 64 input): parameters, logits before and after fuse();
  ls_models.json             the unfused and fused state_dict key lists and parameter counts of recnext_t / _s / _b.
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

# (name, C, stage, H, num_heads, mlp_ratio, seed): the rows of the T / S / B mixer table at 224 (T / S / B share shapes)
BLOCKS = [
    ("28x28_c128", 128, 0, 28, 1, 2, 40),      # B stage 0
    ("14x14_c128", 128, 1, 14, 1, 2, 41),      # T stage 1
    ("14x14_c256", 256, 1, 14, 1, 2, 42),      # S / B stage 1
    ("7x7_c256", 256, 2, 7, 1, 2, 43),         # T stage 2
    ("7x7_c384", 384, 2, 7, 1, 2, 44),         # S / B stage 2
    ("4x4_c512", 512, 3, 4, 2, 1.5, 45),       # T / S / B stage 3 (LinearAttention3)
]


def bf16_bits(t):
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def gen_blocks(refl, out):
    for (name, c, stage, h, heads, ratio, seed) in BLOCKS:
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        blk = refl.MetaNeXtBlock(c, ratio, num_heads=heads, stage=stage).eval()
        make_golden.randomize_bn(blk, gen)
        x = make_golden.bf16_round(torch.randn(1, c, h, h, generator=gen))
        with torch.no_grad():
            r = blk.rep_mixer(x)
            s = blk.token_mixer.split_idx
            t_s = blk.token_mixer.attn(r[:, :s])
        sd = {k: make_golden.np32(v) for k, v in blk.state_dict().items() if v.dtype.is_floating_point and not k.startswith("channel_mixer.")}
        rec = {"x_bf16": bf16_bits(x), "r": make_golden.np32(r), "t_s": make_golden.np32(t_s),
               "meta": np.array(json.dumps(dict(C=c, stage=stage, H=h, W=h, num_heads=heads, mlp_ratio=ratio, split=s, seed=seed)))}
        rec.update({"sd::" + k: v for k, v in sd.items()})
        np.savez(os.path.join(out, f"ls_block_{name}.npz"), **rec)
        print("ls block", name, tuple(t_s.shape))


def gen_tiny(refl, out):
    torch.manual_seed(50)
    gen = torch.Generator().manual_seed(50)
    net = refl.RecNext(embed_dim=(16, 32, 48, 64), depth=(1, 1, 1, 1), mlp_ratios=(2, 2, 2, 1.5), num_heads=(1, 1, 1, 2), split_rates=(4, 4, 4, 4),
                       num_classes=10).eval()
    make_golden.randomize_bn(net, gen)
    x = torch.randn(2, 3, 64, 64, generator=gen)
    with torch.no_grad():
        logits = net(x)
        sd = {k: make_golden.np32(v) for k, v in net.state_dict().items() if v.dtype.is_floating_point}
        net.fuse()
        logits_fused = net(x)
    rec = {"x": make_golden.np32(x), "logits": make_golden.np32(logits), "logits_fused": make_golden.np32(logits_fused)}
    rec.update({"sd::" + k: v for k, v in sd.items()})
    np.savez(os.path.join(out, "ls_tiny_model.npz"), **rec)
    print("ls tiny model", make_golden.np32(logits)[0, :3], f"fuse drift={float((logits - logits_fused).abs().max()):.2e}")


def gen_models(registry, out):
    rec = {}
    for name in ("recnext_t", "recnext_s", "recnext_b"):
        torch.manual_seed(0)
        net = registry[name]().eval()
        keys = list(net.state_dict().keys())
        params = sum(p.numel() for p in net.parameters())
        net.fuse()
        rec[name] = dict(keys=keys, params=params, fused_keys=list(net.state_dict().keys()), fused_params=sum(p.numel() for p in net.parameters()))
        print(name, params, rec[name]["fused_params"])
    with open(os.path.join(out, "ls_models.json"), "w") as f:
        json.dump(rec, f, indent=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.set_num_threads(4)
    registry = make_golden.install_timm_shim()
    refl = make_golden.load_by_path("ref_lsnet_recattn", os.path.join(args.reference, "lsnet", "model", "recattn.py"))
    gen_blocks(refl, args.out)
    gen_tiny(refl, args.out)
    gen_models(registry, args.out)


if __name__ == "__main__":
    main()
