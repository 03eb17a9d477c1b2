"""Downsample.token_mixer of RecNeXt-T / S / B (the grouped 5x5 stride-2 conv): the library's conv against ops.grouped_conv2d (one HIP launch),
bf16, channels_last, the six shapes of the registered models at batch 256 and at batch 1.

    python tools/bench_ls_down.py [--out FILE] [--rounds 5] [--seconds 1.0] [--backward] [--batches 256,1]

--backward measures the conv's backward instead: the library's (autograd of F.conv2d: input and weight gradient, the bias gradient with them)
against ops.grouped_conv2d_backward (rcx_grouped_conv2d_bwd: gx, gw and gb), the compulsory bytes being x and gy in, gx out, the weights in and out.

Both forms run in one process, warmed, in alternating rounds; every round is timed with device events around a run of calls long enough that
the rounds of one form fill about half of --seconds.  Per form: the median round's microseconds a call, the spread (max - min) / median of its
rounds, and the compulsory bytes (x in, y out, the weights once) over the median time.  The copy ceiling these machines have shown is
3.6 - 5.4 TB/s (README, round 6).  A form wins a shape when its median is below the other's by more than the library's own spread."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (model, Cin, Cout, groups, side of the input plane at 224 x 224)
SHAPES = [("T   64->128", 64, 128, 64, 28), ("T  128->256", 128, 256, 128, 14), ("T  256->512", 256, 512, 256, 7),
          ("S/B 128->256", 128, 256, 128, 28), ("S/B 256->384", 256, 384, 128, 14), ("S/B 384->512", 384, 512, 128, 7)]
BATCHES = (256, 1)


def backward_bytes(n, cin, cout, g, side, es=2):
    so = (side + 1) // 2
    return 2 * n * side * side * cin * es + n * so * so * cout * es + 2 * 25 * (cin // g) * cout * 4 + cout * 4
COPY_CEILING = "3.6 - 5.4 TB/s"


def compulsory_bytes(n, cin, cout, g, side, es=2):
    so = (side + 1) // 2
    return n * side * side * cin * es + n * so * so * cout * es + 25 * (cin // g) * cout * 4 + cout * 4


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--seconds", default=1.0, type=float)
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--batches", default=",".join(map(str, BATCHES)))
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    from recnext_amd import ops
    from recnext_amd.build import source_fingerprint
    if not torch.cuda.is_available():
        raise SystemExit("bench_ls_down.py measures on a GPU; there is none")
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
    say("backward: autograd of F.conv2d (gx, gw, gb) against ops.grouped_conv2d_backward" if args.backward else "forward: F.conv2d against ops.grouped_conv2d")
    say(f"device {torch.cuda.get_device_name(0)}; bf16, channels_last; {args.rounds} alternating rounds a form; copy ceiling {COPY_CEILING}")
    say(f"{'shape':14s} {'N':>4s} {'MB':>7s} | {'library us':>10s} {'spread':>7s} {'TB/s':>6s} | {'HIP us':>8s} {'spread':>7s} {'TB/s':>6s} | {'lib/HIP':>7s}  verdict")
    with torch.set_grad_enabled(args.backward):
        for n in (int(v) for v in args.batches.split(",")):
            for label, cin, cout, g, side in SHAPES:
                gen = torch.Generator(device="cpu").manual_seed(cin + side)
                x = torch.randn(n, cin, side, side, generator=gen).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
                w = (torch.randn(cout, cin // g, 5, 5, generator=gen) / 5).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
                b = torch.randn(cout, generator=gen).to(dev).bfloat16()
                wp, bp = ops.pack_grouped_weight(w), b.float()
                assert ops.grouped_conv2d_supported(n, side, side, cin, cout, g, 5, 2, torch.bfloat16)
                if args.backward:
                    assert ops.grouped_conv2d_backward_supported(n, side, side, cin, cout, g, 5, 2, torch.bfloat16)
                    so = (side + 1) // 2
                    gy = torch.randn(n, cout, so, so, generator=gen).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
                    leaves = [t.requires_grad_(True) for t in (x, w, b)]
                    y = F.conv2d(x, w, b, stride=2, padding=2, groups=g)                       # the graph is made once; each call runs its backward
                    forms = {"lib": lambda: torch.autograd.grad(y, leaves, gy, retain_graph=True),
                             "hip": lambda: ops.grouped_conv2d_backward(x, gy, wp, g, need_bias=True)}
                    d = (forms["lib"]()[0].float() - forms["hip"]()[0].float()).abs().max().item()
                else:
                    forms = {"lib": lambda: F.conv2d(x, w, b, stride=2, padding=2, groups=g), "hip": lambda: ops.grouped_conv2d(x, wp, bp, g)}
                    d = (forms["lib"]().float() - forms["hip"]().float()).abs().max().item()   # the same function (bf16 rounding apart)
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
                nbytes = (backward_bytes if args.backward else compulsory_bytes)(n, cin, cout, g, side)
                med = {k: statistics.median(v) for k, v in got.items()}
                spread = {k: (max(v) - min(v)) / med[k] for k, v in got.items()}
                ratio = med["lib"] / med["hip"]
                verdict = "HIP wins" if ratio > 1.0 + spread["lib"] else ("library wins" if ratio < 1.0 - spread["lib"] else "within the spread")
                say(f"{label:14s} {n:4d} {nbytes / 1e6:7.2f} | {med['lib']:10.2f} {spread['lib']:7.1%} {nbytes / med['lib'] / 1e6:6.3f} | "
                    f"{med['hip']:8.2f} {spread['hip']:7.1%} {nbytes / med['hip'] / 1e6:6.3f} | {ratio:7.2f}  {verdict}   (max|lib - HIP| {d:.3g})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
