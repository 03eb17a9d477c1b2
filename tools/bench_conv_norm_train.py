"""The slice mixers' depthwise ConvNorms of a training step, shape by shape: the operator chain of recattn._conv_norm_train / _upadd_conv_norm_train (the
conv's autograd Function, then the module's BatchNorm) against the one-operator form (ops.DwConvBnFn).

    python tools/bench_conv_norm_train.py [--batch 128] [--out FILE] [--rounds 5] [--seconds 0.4] [--trace chain|fused [--calls K]]

The (slice channels, H) of batch-128 T / S / B steps at 224 x 224 (--large: the planes a 448 x 448 step has besides), each in the three forms a RecAttn2d block has -- down[0] (5x5 stride 2 on H), pe (3x3 on
(H + 1) / 2), conv (5x5 on x + nearest-resize(a), on H) -- and LinearAttention3's pe (3x3 on 4 x 4), float32 and bf16 x, forward + backward (gradients of x, of a
and of all four parameters) through the module itself: one lsmodels.ConvNorm in train mode, unmarked (the chain) and marked as
models.use_fused_conv_norm_train(all_shapes=True) marks it (the operator), the same parameters.  Both forms in one process, warmed, in alternating rounds;
a round is a run of calls timed twice over: device events around the run (GPU time; on a host-bound run this is the host's time too) and the wall clock
from the first call to the end of a synchronize.  Per form the median round's microseconds a call and the spread (max - min) / median of its rounds.  A
shape is routed only if the operator's median beats the chain's by more than the chain's own spread in this very job, in wall time and in GPU time.
--trace runs K forward + backward calls of one form at the first shape (bf16) and nothing else: the run to put under a kernel trace; the launches of a
call are the difference of two such traces divided by the difference of their K, which leaves out what the process launches once."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (form, slice channels, H of the tensor the conv reads).  A 224 x 224 step (the stem divides by 8): T's stages 1 - 2, S / B's stages 1 - 2, B's stage 0,
# each as down / pe / conv, and stage 3's pe ...
MIXERS = [(32, 14), (64, 7), (64, 14), (96, 7), (32, 28)]
# ... and, with --large, what a 448 x 448 step has besides
LARGE = [(64, 28), (96, 14), (32, 56)]
FORMS = {"down": (5, 2, False), "pe": (3, 1, False), "conv": (5, 1, True)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default=128, type=int)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--seconds", default=0.4, type=float)
    ap.add_argument("--large", action="store_true", help="the planes of a 448 x 448 step instead")
    ap.add_argument("--trace", default=None, choices=("chain", "fused"))
    ap.add_argument("--calls", default=1, type=int)
    args = ap.parse_args(argv)
    mixers, la3 = (LARGE, 7) if args.large else (MIXERS, 4)
    SHAPES = [(form, c, h if form != "pe" else (h + 1) // 2) for c, h in mixers for form in ("down", "pe", "conv")] + [("pe", 128, la3)]
    import copy
    import torch
    from recnext_amd import lsmodels, recattn
    from recnext_amd.build import source_fingerprint
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_norm_train.py measures on a GPU; there is none")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e6 / iters
        return a.elapsed_time(b) * 1e3 / iters, wall

    def forms(form, c, h, dt):
        k, stride, up = FORMS[form]
        torch.manual_seed(c + h)
        chain = lsmodels.ConvNorm(c, c, kernel_size=k, padding=k // 2, stride=stride, groups=c).to(dev).train()
        fused = copy.deepcopy(chain)
        fused._fused_conv_norm_train = "all"                               # what models.use_fused_conv_norm_train(all_shapes=True) sets
        ho = (h - 1) // stride + 1
        x = (torch.randn(args.batch, h, h, c, device=dev) + 0.3).to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        a = torch.randn(args.batch, (h + 1) // 2, (h + 1) // 2, c, device=dev).permute(0, 3, 1, 2).requires_grad_(True) if up else None
        g = torch.randn(args.batch, ho, ho, c, device=dev).to(dt).permute(0, 3, 1, 2)

        def run(m):
            ps = list(m.parameters())

            def fb():
                y = recattn._upadd_conv_norm_train(m, x, a, "nearest") if up else recattn._conv_norm_train(m, x, stride)
                return torch.autograd.grad(y, [x] + ([a] if up else []) + ps, g)
            return fb
        return {"chain": run(chain), "fused": run(fused)}

    if args.trace:
        form, c, h = SHAPES[0]
        fn = forms(form, c, h, torch.bfloat16)[args.trace]
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        print(f"ran {args.trace} {args.calls} x {form} at C={c}, {args.batch} x {h} x {h}, bf16", flush=True)
        return

    say(f"library_sources_sha256 {source_fingerprint()}")
    say(f"device {torch.cuda.get_device_name(0)}; depthwise ConvNorm forward + backward, batch {args.batch}, channels_last; {args.rounds} alternating rounds a form; "
        f"us a call (median of rounds), spread = (max - min) / median; launches a forward + backward: chain see the kernel trace, fused 3 + 5")
    say(f"{'form':>4s} {'C':>4s} {'H':>3s} {'R':>7s} {'x':>8s} | {'chain gpu':>9s} {'spread':>6s} {'fused gpu':>9s} {'spread':>6s} {'ratio':>5s} | "
        f"{'chain wall':>10s} {'spread':>6s} {'fused wall':>10s} {'spread':>6s} {'ratio':>5s} | verdict")
    for form, c, h in SHAPES:
        for dt in (torch.float32, torch.bfloat16):
            fm = forms(form, c, h, dt)
            ho = (h - 1) // FORMS[form][1] + 1
            iters = {}
            for k, fn in fm.items():
                for _ in range(5):
                    fn()
                iters[k] = max(5, int(args.seconds * 0.5e6 / args.rounds / max(timed(fn, 10)[1], 1.0)))
            got = {k: [] for k in fm}
            for _ in range(args.rounds):
                for k, fn in fm.items():
                    got[k].append(timed(fn, iters[k]))
            med = {k: [statistics.median(t[i] for t in v) for i in (0, 1)] for k, v in got.items()}
            spr = {k: [(max(t[i] for t in v) - min(t[i] for t in v)) / med[k][i] for i in (0, 1)] for k, v in got.items()}
            ratio = [med["chain"][i] / med["fused"][i] for i in (0, 1)]
            wins = all(ratio[i] > 1.0 + spr["chain"][i] for i in (0, 1))
            loses = any(ratio[i] < 1.0 - spr["chain"][i] for i in (0, 1))
            verdict = "fused wins: routed" if wins else ("chain wins: left out" if loses else "within the spread: left out")
            say(f"{form:>4s} {c:4d} {h:3d} {args.batch * ho * ho:7d} {str(dt)[6:]:>8s} | {med['chain'][0]:9.1f} {spr['chain'][0]:6.1%} {med['fused'][0]:9.1f} {spr['fused'][0]:6.1%} {ratio[0]:5.2f} | "
                f"{med['chain'][1]:10.1f} {spr['chain'][1]:6.1%} {med['fused'][1]:10.1f} {spr['fused'][1]:6.1%} {ratio[1]:5.2f} | {verdict}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
