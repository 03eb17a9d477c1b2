#!/usr/bin/env python3
"""One forward + backward of a RecConv2d block with frozen parameters (x requires grad): the launches a kernel-trace profile of the input-only
path sees -- the inference forward and rcx_recconv2d_bwd_input.  Run under `rocprofv3 --kernel-trace --stats -- python3 ...`.
usage: profile_frozen_block.py N C H LEVEL {bf16,f32,f16}"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import recnext_amd
from recnext_amd import build, ops

n, c, h, level = (int(v) for v in sys.argv[1:5])
dtype = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}[sys.argv[5]]
dev = torch.device("cuda:0")
torch.manual_seed(0)
mod = recnext_amd.RecConv2d(c, kernel_size=5, level=level).to(dev).to(dtype)
for p in mod.parameters():
    p.requires_grad_(False)
x = torch.randn(n, c, h, h, device=dev).to(dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True)
g = torch.randn(n, c, h, h, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
torch.cuda.synchronize()
mod(x).backward(g)
torch.cuda.synchronize()
print(json.dumps({"library_sources_sha256": build.source_fingerprint(), "shape": [n, c, h, h], "level": level, "dtype": sys.argv[5],
                  "fwd_plan": ops.recconv2d_plan(n, c, h, h, level, 5, "bilinear", dtype),
                  "bwd_input_plan": ops.recconv2d_bwd_input_plan(n, c, h, h, level, 5, dtype)}))
