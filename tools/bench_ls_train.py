#!/usr/bin/env python3
"""Training step (forward + backward + AdamW) of RecNeXt-T / S / B at 224x224: the HIP token half vs the operator chain (tests/ls_eager.py).

engine.py-style step under bf16 autocast, channels_last, synthetic data; one GPU (development tool, not bench.py).  One JSON line per (model, path)
with the sha256 of the kernel sources it ran on.  --hip-batchnorm reroutes every nn.BatchNorm2d of the model to the HIP BatchNorm
(models.use_hip_batchnorm) before the step; with it, --models also takes the M / A names (recnext_m3 ...) on the HIP token mixers.
--fused-rep runs every RepVGGDW as one HIP operator (models.use_fused_rep_train: the shapes its routing rule keeps; --fused-rep-all: every shape).
--fused-conv-norm runs the slice mixers' depthwise ConvNorms as one HIP operator each (models.use_fused_conv_norm_train; --fused-conv-norm-all: every shape).
--fused-mixer-norms runs the channel mixers' and the stem's BatchNorms with their GELU / residual epilogues (models.use_fused_mixer_norms_train;
--fused-mixer-norms-all: every shape).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recnext_amd import lsmodels, models
from recnext_amd.build import source_fingerprint
from tests.ls_eager import eager_token_mixer

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="recnext_t,recnext_s,recnext_b")
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--which", default="hip,eager")
ap.add_argument("--hip-batchnorm", action="store_true", help="reroute every nn.BatchNorm2d to the HIP BatchNorm (models.use_hip_batchnorm): the shapes its routing rule keeps")
ap.add_argument("--hip-batchnorm-all", action="store_true", help="... and every shape the kernels take, the rule set aside")
ap.add_argument("--fused-rep", action="store_true", help="run every RepVGGDW as one HIP operator (models.use_fused_rep_train): the shapes its routing rule keeps")
ap.add_argument("--fused-rep-all", action="store_true", help="... and every shape the kernels take, the rule set aside")
ap.add_argument("--fused-conv-norm", action="store_true", help="run the slice mixers' depthwise ConvNorms as one HIP operator each (models.use_fused_conv_norm_train): the shapes its routing rule keeps")
ap.add_argument("--fused-conv-norm-all", action="store_true", help="... and every shape the kernels take, the rule set aside")
ap.add_argument("--fused-mixer-norms", action="store_true", help="run the channel mixers' BatchNorm + GELU and BatchNorm + residual as one HIP operator each (models.use_fused_mixer_norms_train): the shapes its routing rule keeps")
ap.add_argument("--fused-mixer-norms-all", action="store_true", help="... and every shape the kernels take, the rule set aside")
args = ap.parse_args()
dev = torch.device("cuda:0")
sha = source_fingerprint()
for name in args.models.split(","):
    for which in args.which.split(","):
        torch.manual_seed(0)
        net = models.create_model(name) if which == "hip" else lsmodels.create_model(name, token_mixer=eager_token_mixer)
        net = net.to(dev).to(memory_format=torch.channels_last).train()
        routed = models.use_hip_batchnorm(net, all_shapes=args.hip_batchnorm_all) if (args.hip_batchnorm or args.hip_batchnorm_all) else 0
        fused_rep = models.use_fused_rep_train(net, all_shapes=args.fused_rep_all) if (args.fused_rep or args.fused_rep_all) else 0
        fused_cn = models.use_fused_conv_norm_train(net, all_shapes=args.fused_conv_norm_all) if (args.fused_conv_norm or args.fused_conv_norm_all) else 0
        fused_mn = models.use_fused_mixer_norms_train(net, all_shapes=args.fused_mixer_norms_all) if (args.fused_mixer_norms or args.fused_mixer_norms_all) else 0
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
        x = torch.randn(args.batch, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 1000, (args.batch,), device=dev)

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = torch.nn.functional.cross_entropy(net(x).float(), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss

        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.steps):
            loss = step()
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / args.steps
        print(json.dumps({"model": name, "token_mixers": which, "hip_batchnorm": routed, "all_shapes": bool(args.hip_batchnorm_all), "fused_rep": fused_rep, "fused_rep_all": bool(args.fused_rep_all), "fused_conv_norm": fused_cn, "fused_conv_norm_all": bool(args.fused_conv_norm_all), "fused_mixer_norms": fused_mn, "fused_mixer_norms_all": bool(args.fused_mixer_norms_all), "batch": args.batch, "steps": args.steps, "ms_per_step": round(ms, 2),
                          "images_per_s": round(args.batch / ms * 1e3, 1), "loss": round(float(loss), 4), "library_sources_sha256": sha}), flush=True)
        del net, opt
        torch.cuda.empty_cache()
