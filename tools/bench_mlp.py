#!/usr/bin/env python3
"""Time the fused channel mixer (rcx_channel_mlp_fwd) against the four library launches it replaces, on the stage shapes of a model at batch 256 (development tool)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from recnext_amd import ops

dev = torch.device("cuda:0")
REPS = int(os.environ.get("REPS", "30"))
ONLY_C = int(os.environ.get("ONLY_C", "0"))              # time the shapes of one channel count alone
ONLY_HIDDEN = [int(v) for v in os.environ.get("ONLY_HIDDEN", "").split(",") if v]       # ... of these hidden widths alone
SHAPES = [(256, 64, 128, 56), (256, 128, 256, 28), (256, 256, 512, 14), (256, 192, 384, 14), (256, 160, 320, 28), (256, 320, 640, 14), (256, 48, 96, 56), (256, 96, 192, 28), (256, 80, 160, 56),
          (256, 512, 1024, 7), (128, 512, 1024, 7), (64, 512, 1024, 7), (32, 512, 1024, 7), (256, 512, 960, 7),   # the 7 x 7 stage, its crossover sweep, A3's padded 960
          (64, 128, 256, 28), (16, 128, 256, 28), (4, 128, 256, 28), (1, 128, 256, 28), (256, 128, 240, 28),   # the resident 128-channel kernel at small M (784 B tokens), A3's padded 240
          (512, 512, 768, 4), (256, 512, 768, 4), (128, 512, 768, 4), (64, 512, 768, 4), (32, 512, 768, 4), (256, 512, 750, 4),   # T / S / B stage 3 (4 x 4), its crossover sweep, a padded 750
          (256, 384, 768, 7), (128, 384, 768, 7), (64, 384, 768, 7), (32, 384, 768, 7), (16, 384, 768, 7), (256, 384, 750, 7)]    # S / B stage 2 and M1 / A1's 7 x 7 stage, likewise


def timed(fn, n):
    for i in range(3):
        fn(i % n)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for i in range(REPS):
        fn(i % n)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / REPS * 1e3


for b, c, hid, hw in SHAPES:
    if (ONLY_C and c != ONLY_C) or (ONLY_HIDDEN and hid not in ONLY_HIDDEN):
        continue
    npool = max(2, int(700e6 / (b * c * hw * hw * 2 * 2)))
    zs = [torch.randn(b, c, hw, hw, device=dev).bfloat16().contiguous(memory_format=torch.channels_last) for _ in range(npool)]
    xs = [torch.randn(b, c, hw, hw, device=dev).bfloat16().contiguous(memory_format=torch.channels_last) for _ in range(npool)]
    w1, b1 = (torch.randn(hid, c, device=dev) * 0.1).bfloat16(), torch.randn(hid, device=dev).bfloat16()
    w2, b2 = (torch.randn(c, hid, device=dev) * 0.1).bfloat16(), torch.randn(c, device=dev).bfloat16()
    m = b * hw * hw
    hp = ops.channel_mlp_hidden(m, c, hid, torch.bfloat16)

    def lib(i):
        zz = zs[i].permute(0, 2, 3, 1).reshape(m, c)
        o = torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(zz, w1, b1)), w2, b2)
        return xs[i] + o.view(b, hw, hw, c).permute(0, 3, 1, 2)

    if not hp:                                       # below the token count the fused kernel is offered from: the library alone
        with torch.no_grad():
            t_l = timed(lib, npool)
        print(json.dumps({"B": b, "C": c, "hidden": hid, "plane": hw, "fused_us": None, "library_us": round(t_l, 1), "note": "no fused kernel at this token count"}))
        continue
    wfrag, bias, hp = ops.pack_channel_mlp(w1, b1, w2, b2, hidden_to=hp)

    with torch.no_grad():
        t_f = timed(lambda i: ops.channel_mlp(zs[i], xs[i], wfrag, bias, hp), npool)
        t_l = timed(lib, npool)
    bytes_ = 3 * m * c * 2
    print(json.dumps({"B": b, "C": c, "hidden": hid, "plane": hw, "fused_us": round(t_f, 1), "library_us": round(t_l, 1), "algorithmic_MB": round(bytes_ / 1e6, 1),
                      "fused_TBs": round(bytes_ / t_f / 1e6, 2), "mfma_TFLOPs": round(4 * m * c * hp / t_f / 1e6, 1)}))
