"""The classifier head (global average pool + linear): the library chain (x.mean((2, 3)) + F.linear) against ops.pool_head (one HIP launch), bf16,
channels_last, the last stage of M0 / M3 / M5 / A3 / T / S at 224 x 224 for batch 1, 8, 64 and 256 and of M3 at 512 x 512 for batch 32 (M3 and A3, and T
and S, end in the same shape: one row each).

    python tools/bench_head.py [--out FILE] [--rounds 5] [--seconds 0.6] [--step-timeout 240]

The parent process never touches the GPU: every shape is one step, a child process of its own under ``timeout``, and the first step that fails ends
the run.  In a step both forms run in one process, warmed, in alternating rounds, measured twice:

  eager   device events around a run of calls from Python, long enough that the rounds of one form fill about half of --seconds: what an eager
          forward pays, the host's side of the two (or one) launches included;
  graph   the same calls captured 20 to a HIP graph and replayed: the GPU's side alone, what a forward under GraphedInference pays.

Per form and measurement: the median round's microseconds a call and the spread (max - min) / median of its rounds.  The HIP launch wins a shape when
its median is below the chain's by more than the chain's own spread, in both measurements; those shapes make head.ROUTED."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (label, C, H, W, batches)
SHAPES = [("M0", 320, 7, 7, (1, 8, 64, 256)), ("M3 / A3", 512, 7, 7, (1, 8, 64, 256)), ("M5", 640, 7, 7, (1, 8, 64, 256)), ("T / S", 512, 4, 4, (1, 8, 64, 256)),
          ("M3 at 512x512", 512, 16, 16, (32,))]
CLASSES = 1000
PER_GRAPH = 20


def worker(index, rounds, seconds):
    import torch
    import torch.nn.functional as F
    from recnext_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("bench_head.py measures on a GPU; there is none")
    dev = torch.device("cuda:0")
    label, c, h, w, batches = SHAPES[index]

    def timed(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / iters                 # microseconds a call

    def graphed(fn):
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(PER_GRAPH):
                fn()
        return g.replay

    def measure(forms, per_call):
        iters = {}
        for k, fn in forms.items():                            # warm, then size the rounds
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            t = timed(fn, 20) / per_call
            iters[k] = max(10, int(seconds * 0.5e6 / rounds / max(t, 1.0) / per_call))
        got = {k: [] for k in forms}
        for _ in range(rounds):
            for k, fn in forms.items():
                got[k].append(timed(fn, iters[k]) / per_call)
        med = {k: statistics.median(v) for k, v in got.items()}
        return med, {k: (max(v) - min(v)) / med[k] for k, v in got.items()}

    with torch.no_grad():
        for n in batches:
            gen = torch.Generator(device="cpu").manual_seed(c + h)
            x = torch.randn(n, c, h, w, generator=gen).to(dev).bfloat16().contiguous(memory_format=torch.channels_last)
            lin = torch.nn.Linear(c, CLASSES).to(dev).bfloat16()
            wpack, bias, _ = ops.pack_head(lin.weight, lin.bias)
            assert ops.pool_head_supported(n, h, w, c, CLASSES, torch.bfloat16)
            forms = {"lib": lambda: F.linear(x.mean((2, 3)), lin.weight, lin.bias), "hip": lambda: ops.pool_head(x, wpack, bias, CLASSES)}
            d = (forms["lib"]().float() - forms["hip"]().float()).abs().max().item()           # the same function (the chain's bf16 mean apart)
            em, es = measure(forms, 1)
            gm, gs = measure({k: graphed(fn) for k, fn in forms.items()}, PER_GRAPH)
            wins = em["lib"] / em["hip"] > 1.0 + es["lib"] and gm["lib"] / gm["hip"] > 1.0 + gs["lib"]
            loses = em["lib"] / em["hip"] < 1.0 - es["lib"] or gm["lib"] / gm["hip"] < 1.0 - gs["lib"]
            verdict = "HIP wins" if wins else ("library wins" if loses else "within the spread")
            print(f"{label:14s} {c:4d} {h:2d}x{w:<2d} {n:4d} | {em['lib']:8.2f} {es['lib']:6.1%} {em['hip']:8.2f} {es['hip']:6.1%} {em['lib'] / em['hip']:6.2f} | "
                  f"{gm['lib']:8.2f} {gs['lib']:6.1%} {gm['hip']:8.2f} {gs['hip']:6.1%} {gm['lib'] / gm['hip']:6.2f} | {verdict}   (max|lib - HIP| {d:.3g})", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--seconds", default=0.6, type=float)
    ap.add_argument("--step-timeout", default=240, type=int, help="seconds a step (one shape, a process of its own) may take")
    ap.add_argument("--worker", default=None, type=int, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.worker is not None:
        return worker(args.worker, args.rounds, args.seconds)
    from recnext_amd.build import source_fingerprint
    lines = [f"library_sources_sha256 {source_fingerprint()}",
             f"x.mean((2, 3)) + F.linear against ops.pool_head; bf16, channels_last, K = {CLASSES}; {args.rounds} alternating rounds a form; graph: {PER_GRAPH} calls a replay",
             f"{'shape':14s} {'C':>4s} {'HxW':>5s} {'N':>4s} | {'eager: lib us':>8s} {'spread':>6s} {'HIP us':>8s} {'spread':>6s} {'lib/HIP':>6s} | "
             f"{'graph: lib us':>8s} {'spread':>6s} {'HIP us':>8s} {'spread':>6s} {'lib/HIP':>6s} | verdict"]
    print("\n".join(lines), flush=True)
    status = 0
    for i in range(len(SHAPES)):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", str(i), "--rounds", str(args.rounds),
               "--seconds", str(args.seconds)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        print(res.stdout, end="", flush=True)
        lines += res.stdout.rstrip("\n").split("\n")
        if res.returncode != 0:                                # a failed, faulted or timed-out step: nothing more is started on the GPU
            lines.append(f"step {SHAPES[i][0]} ended with status {res.returncode}: stopped")
            print(lines[-1], flush=True)
            status = res.returncode
            break
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    raise SystemExit(main())
