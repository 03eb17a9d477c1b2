"""The stem of RecNeXt-T / S / B (three 3x3 stride-2 convs, 3 -> C/4 -> C/2 -> C, a GELU after each): the library's chain against ops.stem3 (two HIP
launches), bf16, channels_last, both channel sets (C = 64: T; C = 128: S / B, with and without the third GELU) at 224 x 224, batch 256 and batch 1.

    python tools/bench_ls_stem.py [--out FILE] [--rounds 5] [--seconds 1.0] [--batches 256,1]

Both forms run in one process, warmed, in alternating rounds; every round is timed with device events around a run of calls long enough that
the rounds of one form fill about half of --seconds.  Per form: the median round's microseconds a call, the spread (max - min) / median of its
rounds, and the compulsory bytes (x in, y out, the weights once) over the median time.  A form wins a shape when its median is below the other's
by more than the library's own spread."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (label, C, GELU after the third conv)
SHAPES = [("T   C=64  +gelu", 64, True), ("S   C=128 +gelu", 128, True), ("B   C=128", 128, False)]
BATCHES = (256, 1)
SIDE = 224


def compulsory_bytes(n, c, side=SIDE, es=2):
    so = -(-side // 8)
    weights = 27 * (c // 4) + 9 * (c // 4) * (c // 2) + 9 * (c // 2) * c
    return n * side * side * 3 * es + n * so * so * c * es + weights * es + (c // 4 + c // 2 + c) * es


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--seconds", default=1.0, type=float)
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    from recnext_amd import ops
    from recnext_amd.build import source_fingerprint
    if not torch.cuda.is_available():
        raise SystemExit("bench_ls_stem.py measures on a GPU; there is none")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / iters                 # microseconds a call

    say(f"library_sources_sha256 {source_fingerprint()}")
    say("forward: F.conv2d / F.gelu chain (three convs) against ops.stem3 (two launches)")
    say(f"device {torch.cuda.get_device_name(0)}; bf16, channels_last, {SIDE} x {SIDE}; {args.rounds} alternating rounds a form")
    say(f"{'shape':16s} {'N':>4s} {'MB':>7s} | {'library us':>10s} {'spread':>7s} {'TB/s':>6s} | {'HIP us':>8s} {'spread':>7s} {'TB/s':>6s} | {'lib/HIP':>7s}  verdict")
    with torch.no_grad():
        for n in (int(v) for v in args.batches.split(",")):
            for label, c, act in SHAPES:
                gen = torch.Generator(device="cpu").manual_seed(c + n)
                x = torch.randn(n, 3, SIDE, SIDE, generator=gen).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
                ws = []
                for cin, cout in ((3, c // 4), (c // 4, c // 2), (c // 2, c)):
                    w = (torch.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
                    ws += [w, (torch.randn(cout, generator=gen) * 0.3).to(dev).bfloat16()]
                pack = ops.pack_stem3(*ws)
                assert ops.stem3_supported(n, SIDE, SIDE, c, act, torch.bfloat16)

                def lib():
                    h = F.gelu(F.conv2d(x, ws[0], ws[1], stride=2, padding=1))
                    h = F.gelu(F.conv2d(h, ws[2], ws[3], stride=2, padding=1))
                    h = F.conv2d(h, ws[4], ws[5], stride=2, padding=1)
                    return F.gelu(h) if act else h

                forms = {"lib": lib, "hip": lambda: ops.stem3(x, *pack, c, act)}
                d = (forms["lib"]().float() - forms["hip"]().float()).abs().max().item()       # the same function (bf16 rounding apart)
                iters = {}
                for k, fn in forms.items():                                                    # warm, then size the rounds
                    for _ in range(10):
                        fn()
                    torch.cuda.synchronize()
                    t = timed(fn, 20)
                    iters[k] = max(10, int(args.seconds * 0.5e6 / args.rounds / max(t, 1.0)))
                got = {"lib": [], "hip": []}
                for _ in range(args.rounds):
                    for k, fn in forms.items():
                        got[k].append(timed(fn, iters[k]))
                nbytes = compulsory_bytes(n, c)
                med = {k: statistics.median(v) for k, v in got.items()}
                spread = {k: (max(v) - min(v)) / med[k] for k, v in got.items()}
                ratio = med["lib"] / med["hip"]
                verdict = "HIP wins" if ratio > 1.0 + spread["lib"] else ("library wins" if ratio < 1.0 - spread["lib"] else "within the spread")
                say(f"{label:16s} {n:4d} {nbytes / 1e6:7.2f} | {med['lib']:10.2f} {spread['lib']:7.1%} {nbytes / med['lib'] / 1e6:6.3f} | "
                    f"{med['hip']:8.2f} {spread['hip']:7.1%} {nbytes / med['hip'] / 1e6:6.3f} | {ratio:7.2f}  {verdict}   (max|lib - HIP| {d:.3g})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
