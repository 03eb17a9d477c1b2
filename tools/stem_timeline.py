#!/usr/bin/env python3
"""Where a tile of the one-launch stem (rcx_stem.hip) spends its cycles: the diagnostic build of that translation unit alone (-DRCX_STEM_STAMPS: s_memtime at
the phase boundaries of every wave, summed over the workgroup's tiles into a buffer of their own), one launch at the RecNeXt-M3 shape (development tool).

    python tools/stem_timeline.py --build            # compile recnext_amd/lib/librcx_stem_diag.so (no GPU needed)
    python tools/stem_timeline.py [--lib PATH]       # run it: cycles per tile, median (p10 - p90) over workgroups, per wave

The stamps fence the schedule (each drains the wave's LDS reads: in this build a pixel tile's gather has landed before the previous one's GELU starts, and the
products are waited for before the GELU's second half, which the product build overlaps), so read the SHARES, not the length, of this build.  In phase A a wave
gathers and multiplies three pixel tiles and takes 2.5 of them through GELU and write (the last round is shared by the waves of a pair)."""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIAG = os.path.join(ROOT, "recnext_amd", "lib", "librcx_stem_diag.so")
SEGMENTS = ["x tile -> LDS (+ wait for x)", "wait at barrier 1", "A gather (LDS reads back)", "A products", "A bias + GELU", "A convert + h1 write", "wait at barrier 2",
            "request next x", "B products (reads + MFMA)", "B bias + stores"]
NS = len(SEGMENTS)                                                       # the kernel's tsum[NS] counts the tiles a workgroup walked


def build():
    src = os.path.join(ROOT, "recnext_amd", "csrc")
    os.makedirs(os.path.dirname(DIAG), exist_ok=True)
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Xclang", "-target-feature", "-Xclang", "-load-store-opt",
           "-DRCX_STEM_STAMPS", "-I", src, "-shared", os.path.join(src, "rcx_stem.hip"), "-o", DIAG]
    subprocess.check_call(cmd)
    print("built", DIAG)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--lib", default=DIAG)
    ap.add_argument("--shape", default="256,32,64,224,224", help="N,CM,CO,H,W")
    a = ap.parse_args()
    if a.build:
        return build()
    import torch
    from recnext_amd import ops
    n, cm, co, h, w = map(int, a.shape.split(","))
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    rb = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(torch.bfloat16).to(dev)
    x = rb(n, 3, h, w).contiguous(memory_format=torch.channels_last)
    pack = ops.pack_stem(rb(cm, 3, 3, 3, sc=(2.0 / 27) ** 0.5), rb(cm, sc=0.3), rb(co, cm, 3, 3, sc=(2.0 / (9 * cm)) ** 0.5), rb(co, sc=0.3))
    ref = ops.stem(x, *pack, cm, co)                                     # the product build: the diagnostic build must compute the same
    y = torch.empty_like(ref)
    lib = ctypes.CDLL(a.lib)
    lib.rcx_stem_diag_fwd.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    stamps = torch.zeros(4 * cus, 4, NS + 1, dtype=torch.int64, device=dev)  # at most four workgroups per compute unit
    torch.cuda.synchronize()
    for _ in range(3):                                                   # warm: the last launch's stamps are read
        stamps.zero_()
        rc = lib.rcx_stem_diag_fwd(x.data_ptr(), y.data_ptr(), *(p.data_ptr() for p in pack), n, h, w, cm, co, stamps.data_ptr(), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
    print(f"stem timeline, N={n} CM={cm} CO={co} {h}x{w}: diagnostic output {'identical to' if torch.equal(y, ref) else 'DIFFERS from'} the product build's")
    s = stamps.cpu().double()
    s = s[s[:, 0, NS] > 0]                                               # workgroups that ran
    tiles = s[:, :, NS:NS + 1]
    per = s[:, :, :NS] / tiles                                            # cycles per tile
    print(f"{s.shape[0]} workgroups, {float(tiles[:, 0, 0].median()):.1f} tiles each (median); cycles per tile of one wave: median (p10 - p90) over workgroups")
    q = lambda t, p: float(torch.quantile(t, p))
    for k, name in enumerate(SEGMENTS):
        row = "  ".join(f"w{wv} {q(per[:, wv, k], .5):7.0f} ({q(per[:, wv, k], .1):5.0f}-{q(per[:, wv, k], .9):5.0f})" for wv in range(4))
        print(f"  {name:32s} {row}")
    tot = per.sum(dim=2)
    print(f"  {'sum':32s} " + "  ".join(f"w{wv} {q(tot[:, wv], .5):7.0f}{'':14s}" for wv in range(4)))
    mean = per.mean(dim=1)
    print("  mean over the four waves, share of the tile: " + ", ".join(f"{name.split(' (')[0]} {100 * q(mean[:, k], .5) / q(tot.mean(dim=1), .5):.1f} %" for k, name in enumerate(SEGMENTS)))


if __name__ == "__main__":
    main()
