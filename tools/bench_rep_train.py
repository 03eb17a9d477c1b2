"""RepVGGDW of a training step, shape by shape: the operator chain of lsmodels._rep_train against the one-operator form (ops.RepDwFn).

    python tools/bench_rep_train.py [--batch 128] [--out FILE] [--rounds 5] [--seconds 0.4] [--trace chain|fused [--calls K]]

Six (C, H) of batch-128 T / S / B steps and the four more that a 224 x 224 step has, float32 and bf16 x, forward + backward (gradients of x and of all eight parameters) through the module
itself: one lsmodels.RepVGGDW in train mode, unmarked (the chain) and marked by models.use_fused_rep_train(all_shapes=True) (the operator), the same
parameters.  Both forms in one process, warmed, in alternating rounds; a round is a run of calls timed twice over: device events around the run (GPU
time; on a host-bound run this is the host's time too) and the wall clock from the first call to the end of a synchronize.  Per form the median
round's microseconds a call and the spread (max - min) / median of its rounds.  A shape stays routed only if the operator's median beats the chain's by
more than the chain's own spread in this very job, in wall time and in GPU time.  --trace runs K forward + backward calls of one form at the first
shape (bf16) and nothing else: the run to put under a kernel trace; the launches of a call are the difference of two such traces divided by the
difference of their K, which leaves out what the process launches once."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(128, 28), (128, 14), (256, 14), (256, 7), (384, 7), (512, 4)]
# ... and what a 224 x 224 step has besides: S / B's 128 x 56^2, 256 x 28^2 and 384 x 14^2, and the 512 x 7^2 of all three
SHAPES += [(128, 56), (256, 28), (384, 14), (512, 7)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default=128, type=int)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--seconds", default=0.4, type=float)
    ap.add_argument("--trace", default=None, choices=("chain", "fused"))
    ap.add_argument("--calls", default=1, type=int)
    args = ap.parse_args(argv)
    import copy
    import torch
    from recnext_amd import lsmodels, models
    from recnext_amd.build import source_fingerprint
    if not torch.cuda.is_available():
        raise SystemExit("bench_rep_train.py measures on a GPU; there is none")
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

    def forms(c, h, dt):
        torch.manual_seed(c + h)
        chain = lsmodels.RepVGGDW(c).to(dev).train()
        fused = copy.deepcopy(chain)
        models.use_fused_rep_train(fused, all_shapes=True)
        x = (torch.randn(args.batch, h, h, c, device=dev) + 0.3).to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        g = torch.randn(args.batch, h, h, c, device=dev).permute(0, 3, 1, 2)

        def run(m):
            ps = list(m.parameters())

            def fb():
                r = lsmodels._rep_train(m, x)
                return torch.autograd.grad(r, [x] + ps, g if r.dtype == g.dtype else g.to(r.dtype))
            return fb
        return {"chain": run(chain), "fused": run(fused)}

    if args.trace:
        c, h = SHAPES[0]
        fn = forms(c, h, torch.bfloat16)[args.trace]
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        print(f"ran {args.trace} {args.calls} x at C={c}, {args.batch} x {h} x {h}, bf16", flush=True)
        return

    say(f"library_sources_sha256 {source_fingerprint()}")
    say(f"device {torch.cuda.get_device_name(0)}; RepVGGDW forward + backward, batch {args.batch}, channels_last; {args.rounds} alternating rounds a form; "
        f"us a call (median of rounds), spread = (max - min) / median; launches a forward + backward: chain see the kernel trace, fused 3 + 4")
    say(f"{'C':>4s} {'H':>3s} {'R':>7s} {'x':>8s} | {'chain gpu':>9s} {'spread':>6s} {'fused gpu':>9s} {'spread':>6s} {'ratio':>5s} | "
        f"{'chain wall':>10s} {'spread':>6s} {'fused wall':>10s} {'spread':>6s} {'ratio':>5s} | verdict")
    for c, h in SHAPES:
        for dt in (torch.float32, torch.bfloat16):
            fm = forms(c, h, dt)
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
            say(f"{c:4d} {h:3d} {args.batch * h * h:7d} {str(dt)[6:]:>8s} | {med['chain'][0]:9.1f} {spr['chain'][0]:6.1%} {med['fused'][0]:9.1f} {spr['fused'][0]:6.1%} {ratio[0]:5.2f} | "
                f"{med['chain'][1]:10.1f} {spr['chain'][1]:6.1%} {med['fused'][1]:10.1f} {spr['fused'][1]:6.1%} {ratio[1]:5.2f} | {verdict}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
