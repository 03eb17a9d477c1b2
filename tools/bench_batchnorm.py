"""The BatchNorms of a model's training step, shape by shape: the library's F.batch_norm against the HIP BatchNorm (ops.BatchNormFn).

    python tools/bench_batchnorm.py [--model recnext_s[,recnext_t,...]] [--batch 128] [--out FILE] [--rounds 5] [--seconds 0.4] [--fp32]

The census is taken with forward hooks on every nn.BatchNorm2d during one training-mode forward under bf16 autocast (channels_last, 224 x 224): the
distinct (N, H, W, C, dtype) and how many BatchNorms of the step have each.  For each distinct shape, forward alone and forward + backward are timed
for both forms in one process, warmed, in alternating rounds, each round timed with device events around a run of calls; per form the median round's
microseconds a call and the spread (max - min) / median of its rounds.  A shape stays routed only if HIP's median beats the library's by more than
the library's own spread, forward + backward; the library's figure of this very job is the yardstick.  Launches a call: the library's from the
profile of the training step (3 forward, 3 backward), HIP's from its launch sequence."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def census(name, batch, dev, autocast):
    import torch
    import torch.nn as nn
    from recnext_amd import models
    torch.manual_seed(0)
    net = models.create_model(name).to(dev).to(memory_format=torch.channels_last).train()
    seen = {}

    def hook(mod, inp, out):
        x = inp[0]
        if x.dim() == 4:
            n, c, h, w = x.shape
            dense = x.is_contiguous(memory_format=torch.channels_last) or (h == 1 and w == 1 and x.is_contiguous())
            key = (n, h, w, c, x.dtype, dense)
            seen[key] = seen.get(key, 0) + 1
    hooks = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, nn.BatchNorm2d)]
    x = torch.randn(batch, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        net(x)
    for h in hooks:
        h.remove()
    del net
    torch.cuda.empty_cache()
    return seen


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="recnext_s")
    ap.add_argument("--batch", default=128, type=int)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--seconds", default=0.4, type=float)
    ap.add_argument("--fp32", action="store_true", help="the census without autocast (float32 activations)")
    args = ap.parse_args(argv)
    import torch
    import torch.nn.functional as F
    from recnext_amd import _lib, ops
    from recnext_amd.build import source_fingerprint
    if not torch.cuda.is_available():
        raise SystemExit("bench_batchnorm.py measures on a GPU; there is none")
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
        return a.elapsed_time(b) * 1e3 / iters

    say(f"library_sources_sha256 {source_fingerprint()}")
    say(f"device {torch.cuda.get_device_name(0)}; channels_last, 224 x 224, batch {args.batch}, {'float32' if args.fp32 else 'bf16 autocast'}; "
        f"{args.rounds} alternating rounds a form; us a call (median of rounds), spread = (max - min) / median")
    shapes = {}
    for name in args.model.split(","):
        seen = census(name, args.batch, dev, not args.fp32)
        say(f"census {name}: {sum(seen.values())} BatchNorm2d calls a step, {len(seen)} distinct shapes, "
            f"{sum(v for k, v in seen.items() if not k[3])} on input that is not dense channels_last")
        for (n, h, w, c, dt, dense), cnt in seen.items():
            if dense:
                shapes.setdefault((n, h, w, c, dt), {})[name] = cnt
    say(f"{'N x H x W':>13s} {'R':>8s} {'C':>5s} {'dtype':>8s} {'MB':>7s} | {'lib fwd':>8s} {'spread':>6s} {'HIP fwd':>8s} {'spread':>6s} {'ratio':>5s} | "
        f"{'lib f+b':>8s} {'spread':>6s} {'HIP f+b':>8s} {'spread':>6s} {'ratio':>5s} | launches lib 3+3, HIP 3+3 | verdict (f+b) | uses")
    for (n, h, wd, c, dt), uses in sorted(shapes.items(), key=lambda kv: (-kv[0][0] * kv[0][1] * kv[0][2] * kv[0][3] * (4 if kv[0][4] == torch.float32 else 2), kv[0][3])):
        r = n * h * wd
        gen = torch.Generator(device="cpu").manual_seed(r + c)
        x = (torch.randn(n, h, wd, c, generator=gen) + 0.3).to(dev).to(dt).permute(0, 3, 1, 2)                 # dense NHWC, the step's own extents
        gy = torch.randn(n, h, wd, c, generator=gen).to(dev).to(dt).permute(0, 3, 1, 2)
        w = (torch.rand(c, generator=gen) + 0.5).to(dev).requires_grad_(True)
        b = torch.randn(c, generator=gen).to(dev).requires_grad_(True)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        xg = x.detach().requires_grad_(True)
        if not _lib.load().rcx_batchnorm_workspace_bytes(n, h, wd, c, ops._DT[dt]):
            say(f"{n:4d}x{h:3d}x{wd:3d} {r:8d} {c:5d} {str(dt)[6:]:>8s}: no kernel")
            continue

        def lib_f():
            with torch.no_grad():
                return F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5)

        def hip_f():
            return ops.batch_norm_train(x, w.detach(), b.detach(), rm, rv, 0.1, 1e-5)[0]

        def lib_fb():
            y = F.batch_norm(xg, rm, rv, w, b, True, 0.1, 1e-5)
            return torch.autograd.grad(y, (xg, w, b), gy)

        def hip_fb():
            y = ops.BatchNormFn.apply(xg, w, b, rm, rv, True, 0.1, 1e-5)
            return torch.autograd.grad(y, (xg, w, b), gy)

        res = {}
        for tag, forms in (("f", {"lib": lib_f, "hip": hip_f}), ("fb", {"lib": lib_fb, "hip": hip_fb})):
            iters = {}
            for k, fn in forms.items():
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                t = timed(fn, 10)
                iters[k] = max(5, int(args.seconds * 0.5e6 / args.rounds / max(t, 1.0)))
            got = {"lib": [], "hip": []}
            for _ in range(args.rounds):
                for k, fn in forms.items():
                    got[k].append(timed(fn, iters[k]))
            med = {k: statistics.median(v) for k, v in got.items()}
            res[tag] = (med, {k: (max(v) - min(v)) / med[k] for k, v in got.items()})
        (mf, sf), (mb, sb) = res["f"], res["fb"]
        ratio = mb["lib"] / mb["hip"]
        verdict = "HIP wins" if ratio > 1.0 + sb["lib"] else ("library wins" if ratio < 1.0 - sb["lib"] else "within the spread")
        say(f"{n:4d}x{h:3d}x{wd:3d} {r:8d} {c:5d} {str(dt)[6:]:>8s} {r * c * x.element_size() / 1e6:7.2f} | {mf['lib']:8.1f} {sf['lib']:6.1%} {mf['hip']:8.1f} {sf['hip']:6.1%} {mf['lib'] / mf['hip']:5.2f} | "
            f"{mb['lib']:8.1f} {sb['lib']:6.1%} {mb['hip']:8.1f} {sb['hip']:6.1%} {ratio:5.2f} | {verdict:17s} | " + ", ".join(f"{k} x{v}" for k, v in uses.items()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
