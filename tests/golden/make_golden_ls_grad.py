#!/usr/bin/env python3
"""Generate the RecNeXt-T / S / B training fixtures (tests/golden/ls_grad_*.npz) by IMPORTING the reference (build container only).

    python tests/golden/make_golden_ls_grad.py [--reference /root/reference]

Runs one lsnet/model/recattn.py MetaNeXtBlock per slice-mixer form of the T / S / B table in TRAIN mode in float64 on torch CPU, under
make_golden.py's timm shim, and stores data only.  The token half is what is pinned: t = cat(mixer(r[:, :s]), r[:, s:]) with r = rep_mixer(x), the
loss <gy, t>.  (The channel mixer is a pair of library 1x1 convs; its 512-channel weights alone would exceed the size limit of a fixture.)
Files are named ls_grad_s<stage>_<plane>_c<C>.npz by what they hold.  Stage, C and heads are the table's; where the table's plane would not fit a
batch of 2 well under 1 MB the plane or C is smaller (s1_9x9_c256 stands for 14 x 14 x 256; s0_28x28_c32 pins stage 0's 28 x 28 plane, whose
14 x 14 = 196-token attention plane no other row has, on a 32-channel block): the semantics pinned -- BatchNorm on batch statistics, the running-
statistics update, every gradient -- do not depend on either.
Each file holds
  x (2, C, H, W) and gy (the shape of t), both float64 values rounded to bf16 (stored as bf16 bits);
  sd::<key>     the rep_mixer / token_mixer parameters and buffers before the step (non-trivial BatchNorm statistics), float32 (exact: the
                block is made in float32, then run in float64);
  t, gx         the token half's output and dL/dx, float32;
  grad::<name>  dL/d<parameter> for every rep_mixer / token_mixer parameter, float32;
  run::<key>    the BatchNorm running statistics after the step, float64;
  meta          JSON: C, stage, H, W, num_heads, mlp_ratio, split, seed.
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

# (name, C, stage, H, num_heads, mlp_ratio, seed)
ROWS = [
    ("s0_28x28_c32", 32, 0, 28, 1, 2, 140),       # B stage 0 (28 x 28, attention plane 14 x 14), on 32 channels
    ("s1_14x14_c128", 128, 1, 14, 1, 2, 141),     # T stage 1
    ("s1_9x9_c256", 256, 1, 9, 1, 2, 142),         # S / B stage 1 (14 x 14 at 224; an odd plane)
    ("s2_7x7_c256", 256, 2, 7, 1, 2, 143),        # T stage 2
    ("s2_7x7_c384", 384, 2, 7, 1, 2, 144),        # S / B stage 2 (96-wide heads)
    ("s3_4x4_c512", 512, 3, 4, 2, 1.5, 145),      # T / S / B stage 3 (LinearAttention3)
]
BATCH = 2


def gen(refl, out):
    for (name, c, stage, h, heads, ratio, seed) in ROWS:
        torch.manual_seed(seed)
        g = torch.Generator().manual_seed(seed)
        blk = refl.MetaNeXtBlock(c, ratio, num_heads=heads, stage=stage)
        make_golden.randomize_bn(blk, g)
        blk = blk.double().train()
        s = blk.token_mixer.split_idx
        x = make_golden.bf16_round(torch.randn(BATCH, c, h, h, generator=g)).double().requires_grad_()
        sd = {k: v.detach().clone() for k, v in blk.state_dict().items() if not k.startswith("channel_mixer.") and v.dtype.is_floating_point}
        with torch.enable_grad():
            r = blk.rep_mixer(x)
            t = torch.cat([blk.token_mixer.attn(r[:, :s]), r[:, s:]], dim=1)
            gy = make_golden.bf16_round(torch.randn(t.shape, generator=g)).double()
            (t * gy).sum().backward()
        rec = {"x_bf16": bf16_bits(x.detach().float()), "gy_bf16": bf16_bits(gy.float()), "t": make_golden.np32(t), "gx": make_golden.np32(x.grad),
               "meta": np.array(json.dumps(dict(C=c, stage=stage, H=h, W=h, num_heads=heads, mlp_ratio=ratio, split=s, seed=seed)))}
        rec.update({"sd::" + k: v.float().numpy() for k, v in sd.items()})
        for k, p in blk.named_parameters():
            if not k.startswith("channel_mixer."):
                assert p.grad is not None, k
                rec["grad::" + k] = make_golden.np32(p.grad)
        rec.update({"run::" + k: v.detach().numpy().copy() for k, v in blk.state_dict().items()
                    if not k.startswith("channel_mixer.") and (k.endswith("running_mean") or k.endswith("running_var"))})
        path = os.path.join(out, f"ls_grad_{name}.npz")
        np.savez(path, **rec)
        print("ls grad", name, f"{h}x{h}", tuple(t.shape), f"{os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    torch.set_num_threads(4)
    make_golden.install_timm_shim()
    refl = make_golden.load_by_path("ref_lsnet_recattn", os.path.join(args.reference, "lsnet", "model", "recattn.py"))
    gen(refl, args.out)


if __name__ == "__main__":
    main()
