#!/usr/bin/env python3
"""Where a hidden step of the channel-mixer ring kernels (rcx_mlp.hip) spends its cycles: the diagnostic build of that translation unit alone (-DRCX_MLP_STAMPS:
s_memtime at the phase boundaries of a hidden step of every wave, summed into a buffer of this tool's own), one launch per kernel at its RecNeXt-M3 shape
(development tool).

    python tools/mlp_timeline.py --build [--form parent|pinned]    # compile recnext_amd/lib/librcx_mlp_diag_<form>.so (no GPU needed)
    python tools/mlp_timeline.py [--form parent|pinned]            # run it: cycles per hidden step, median (p10 - p90) over waves

--form parent builds every caller in hidden_tile_ring's form as the compiler schedules it (-DRCX_MLP_PINNED=false), pinned the form the library ships (they differ in
k_channel_mlp_pair alone).  Under the stamps hidden_tile_ring requests W2's first fragments behind the GELU; the product build sends one of them in front of it.
The stamps fence the schedule (each drains the wave's LDS reads, so a request kept in flight across a phase boundary in the product build is paid in the phase that
issued it), so read the SHARES, not the length, of this build."""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PHASES = ["ring preload", "D1 products", "b1 + GELU", "D2 products", "barrier / DMA wait"]
# (kernel, batch, channels, hidden, plane) at RecNeXt-M3, 224 x 224, batch 256
SHAPES = [("k_channel_mlp_pair (14x14, C=256)", 256, 256, 512, 14), ("k_channel_mlp_res128 (28x28, C=128)", 256, 128, 256, 28), ("k_channel_mlp (56x56, C=64)", 256, 64, 128, 56)]


def diag_path(form):
    return os.path.join(ROOT, "recnext_amd", "lib", f"librcx_mlp_diag_{form}.so")


def build(form):
    src = os.path.join(ROOT, "recnext_amd", "csrc")
    os.makedirs(os.path.dirname(diag_path(form)), exist_ok=True)
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Xclang", "-target-feature", "-Xclang", "-load-store-opt",
           "-DRCX_MLP_STAMPS", "-DRCX_MLP_PINNED=" + ("true" if form == "pinned" else "false"), "-I", src, "-shared", os.path.join(src, "rcx_mlp.hip"), "-o", diag_path(form)]
    subprocess.check_call(cmd)
    print("built", diag_path(form))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--form", choices=["parent", "pinned"], default="pinned")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.build:
        return build(a.form)
    import torch
    from recnext_amd import ops
    dev = torch.device("cuda:0")
    lib = ctypes.CDLL(a.lib or diag_path(a.form))
    lib.rcx_mlp_diag_fwd.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    q = lambda t, p: float(torch.quantile(t, p))
    print(f"channel-mixer timeline, form = {a.form}: cycles (s_memtime ticks) per hidden step of one wave, median (p10 - p90) over the waves that ran")
    for name, b, c, hid, hw in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(0)
        rb = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(torch.bfloat16).to(dev)
        z = rb(b, c, hw, hw).contiguous(memory_format=torch.channels_last)
        x = rb(b, c, hw, hw).contiguous(memory_format=torch.channels_last)
        m = b * hw * hw
        hp = ops.channel_mlp_hidden(m, c, hid, torch.bfloat16)
        wfrag, bias, hp = ops.pack_channel_mlp(rb(hid, c, sc=0.1), rb(hid), rb(c, hid, sc=0.1), rb(c), hidden_to=hp)
        ref = ops.channel_mlp(z, x, wfrag, bias, hp)                     # the product build: the diagnostic build must compute the same
        y = torch.empty_like(ref)
        stamps = torch.zeros(16 * cus, 8, dtype=torch.int64, device=dev)  # at most 12 waves a workgroup, one workgroup a compute unit
        torch.cuda.synchronize()
        for _ in range(3):                                               # warm: the last launch's stamps are read
            stamps.zero_()
            rc = lib.rcx_mlp_diag_fwd(z.data_ptr(), x.data_ptr(), y.data_ptr(), wfrag.data_ptr(), bias.data_ptr(), m, c, hp, stamps.data_ptr(), None)
            assert rc == 0, rc
            torch.cuda.synchronize()
        s = stamps.cpu().double()
        s = s[s[:, 6] > 0]                                               # waves that ran a hidden step
        per = s[:, :5] / s[:, 6:7]
        rest = s[:, 5] / s[:, 6]
        print(f"== {name}: {s.shape[0]} waves, {q(s[:, 6], .5):.0f} hidden steps each (median); diagnostic output "
              f"{'identical to' if torch.equal(y, ref) else 'DIFFERS from'} the product build's")
        tot = per.sum(dim=1)
        for k, ph in enumerate(PHASES):
            print(f"  {ph:22s} {q(per[:, k], .5):8.0f} ({q(per[:, k], .1):6.0f} - {q(per[:, k], .9):6.0f})   {100 * q(per[:, k], .5) / q(tot, .5):5.1f} % of the step")
        print(f"  {'hidden step, sum':22s} {q(tot, .5):8.0f} ({q(tot, .1):6.0f} - {q(tot, .9):6.0f})")
        print(f"  {'tile prologue/epilogue':22s} {q(rest, .5):8.0f} per hidden step (outside the steps: z staging, residual, stores)")


if __name__ == "__main__":
    main()
