#!/usr/bin/env python3
"""Generate the large-plane token-half fixtures of the LSNet-style RecNeXt-T / S / B (tests/golden/ls_tiled_block_*) by IMPORTING the reference
(build container only).

    python tests/golden/make_golden_ls_tiled.py [--reference /root/reference]

Same recipe and record as make_golden_ls.py's ls_block_* files (its helpers are imported, the script itself is untouched), on planes the
one-workgroup HIP entries refuse: more than 64 tokens for LinearAttention3, images past the LDS for RecAttn2d, odd and non-square planes.  The
files carry another prefix so that the ls_block_* case list of the existing tests stays as it is.  To keep every file below the largest ls_block_*
one, `r` is stored for the channels [0, meta["r_channels"]) only: the whole of it where that fits, else the slice and the first four passthrough
channels (RepVGGDW is depthwise: every channel is computed alike).
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
import make_golden_ls  # noqa: E402

# (name, C, stage, H, W, num_heads, mlp_ratio, seed)
BLOCKS = [
    ("12x12_c512", 512, 3, 12, 12, 2, 1.5, 60),       # stage 3 (LinearAttention3) of a 384 x 384 input
    ("9x13_c512", 512, 3, 9, 13, 2, 1.5, 61),         # LinearAttention3, odd and non-square
    ("36x36_c128", 128, 0, 36, 36, 1, 2, 62),         # B stage 0 of a 288 x 288 input
    ("16x16_c384", 384, 2, 16, 16, 1, 2, 63),         # S / B stage 2 of a 256 x 256 input: the 96-wide slice
    ("25x19_c256", 256, 1, 25, 19, 1, 2, 64),         # RecAttn2d, odd and non-square (13 x 10 half-size plane)
]
WHOLE_R_LIMIT = 560_000          # bytes of x (bf16) + r + t_s (float32) up to which r is stored whole


def gen_blocks(refl, out):
    for (name, c, stage, h, w, heads, ratio, seed) in BLOCKS:
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(seed)
        blk = refl.MetaNeXtBlock(c, ratio, num_heads=heads, stage=stage).eval()
        make_golden.randomize_bn(blk, gen)
        x = make_golden.bf16_round(torch.randn(1, c, h, w, generator=gen))
        with torch.no_grad():
            r = blk.rep_mixer(x)
            s = blk.token_mixer.split_idx
            t_s = blk.token_mixer.attn(r[:, :s])
        rc = c if h * w * (2 * c + 4 * c + 4 * s) <= WHOLE_R_LIMIT else s + 4
        sd = {k: make_golden.np32(v) for k, v in blk.state_dict().items() if v.dtype.is_floating_point and not k.startswith("channel_mixer.")}
        rec = {"x_bf16": make_golden_ls.bf16_bits(x), "r": make_golden.np32(r[:, :rc]), "t_s": make_golden.np32(t_s),
               "meta": np.array(json.dumps(dict(C=c, stage=stage, H=h, W=w, num_heads=heads, mlp_ratio=ratio, split=s, seed=seed, r_channels=rc)))}
        rec.update({"sd::" + k: v for k, v in sd.items()})
        path = os.path.join(out, f"ls_tiled_block_{name}.npz")
        np.savez(path, **rec)
        print("ls tiled block", name, tuple(t_s.shape), "r channels", rc, os.path.getsize(path), "bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.set_num_threads(4)
    make_golden.install_timm_shim()
    refl = make_golden.load_by_path("ref_lsnet_recattn", os.path.join(args.reference, "lsnet", "model", "recattn.py"))
    gen_blocks(refl, args.out)


if __name__ == "__main__":
    main()
