#!/usr/bin/env python3
"""Wide linear-attention core (rcx_linear_attention_wide_fwd / _bwd) alone, per batch size: does one workgroup per (image, head) leave the GPU
underfilled at the batches a training step uses?  One JSON line per (head shape, batch): microseconds per forward and per backward call
(host time included; run it under `rocprofv3 --kernel-trace --stats` for the kernels' device time).

    python tools/bench_wide_core.py [--batches 32,64,128,256,512] [--iters 200] [--head sb_stage2,stage3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recnext_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="32,64,128,256,512")
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--head", default="sb_stage2,stage3", help="which head shapes (a kernel trace of one shape and batch gives the launch's device time)")
args = ap.parse_args()
dev = torch.device("cuda:0")
# (label, Dk, Dv, plane) of the T / S / B heads that take the wide core at 224 x 224: S / B stage 2 (attention plane 4 x 4), stage 3 (4 x 4)
SHAPES = [("sb_stage2", 96, 96, 4), ("stage3", 64, 128, 4)]


def timed(fn):
    for _ in range(5):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(args.iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / args.iters


for label, dk, dv, side in [sh for sh in SHAPES if sh[0] in args.head.split(",")]:
    for b in map(int, args.batches.split(",")):
        n = side * side
        mk = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16)
        qpre, kpre = mk(b, n, dk), mk(b, n, dk)
        v, pe, g = (mk(b, dv, side, side).contiguous(memory_format=torch.channels_last) for _ in range(3))
        fwd = timed(lambda: ops.linear_attention_wide(qpre, kpre, v, pe, 1))
        bwd = timed(lambda: ops.linear_attention_wide_backward(qpre, kpre, v, g, 1))
        print(json.dumps({"head": label, "dk": dk, "dv": dv, "tokens": n, "batch": b, "workgroups": b, "dtype": "bf16",
                          "us_fwd": round(fwd, 2), "us_bwd": round(bwd, 2), "ns_per_image_fwd_bwd": round((fwd + bwd) * 1e3 / b, 1)}), flush=True)
