"""The channel mixers' (and the stems') BatchNorms of a training step with their epilogues, shape by shape: the operator chain -- F.batch_norm + F.gelu, and
F.batch_norm, the DropPath mask multiply and the residual add -- against the one-operator forms (ops.BnGeluFn, ops.BnAddFn), then the step itself.

    python tools/bench_mixer_norms_train.py [--batch 128] [--models recnext_m3,recnext_t,recnext_s,recnext_b] [--out FILE] [--rounds 5] [--seconds 0.3]
                                            [--steps-of recnext_t,recnext_s] [--memory-of recnext_s]

The census of (R x C, dtype of u, epilogue, dtype of the residual) comes from a training-mode forward of every model at the batch, in float32 and under
bf16 autocast, with hooks on the mixers' and stems' BatchNorms (the tensor each norm is given) and on their hosts (the residual's dtype is the block's
output's).  Each entry: forward + backward (gradients of u, of r and of both parameters) of the chain and of the operator in one process, warmed, in
alternating rounds; a round is a run of calls timed twice over: device events around the run (GPU time; on a host-bound run the host's too) and the wall
clock from the first call to the end of a synchronize.  Per form the median round's microseconds a call and the spread (max - min) / median of its
rounds.  A shape is routed only if the operator's median beats the chain's by more than the chain's own spread in this very job and by at least --margin (a
tenth: the operator costs the host more than the chain does, so a smaller win of the isolated call is a loss in a host-bound step), in wall time and in
GPU time; the table the binding would take from this job alone (half to twice the measured rows) is printed at the end.
--steps-of: the training step (bf16 autocast, AdamW) of each model, unmarked and marked (all_shapes; and by the routing rule where the table is not
empty), alternated off / on twice in one process: milliseconds a step, and whether the change exceeds the off-runs' spread.  --memory-of: the peak
torch.cuda.max_memory_allocated of one such step, off and on."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default=128, type=int)
    ap.add_argument("--models", default="recnext_m3,recnext_t,recnext_s,recnext_b")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--seconds", default=0.3, type=float)
    ap.add_argument("--steps-of", default="")
    ap.add_argument("--memory-of", default="")
    ap.add_argument("--steps", default=6, type=int)
    ap.add_argument("--margin", default=0.10, type=float, help="the least win that routes a shape, where the chain's spread is smaller")
    args = ap.parse_args(argv)
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from recnext_amd import bnact, lsmodels, models, ops
    from recnext_amd.build import source_fingerprint
    from recnext_amd.layers import ConvNorm
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixer_norms_train.py measures on a GPU; there is none")
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def build(name):
        torch.manual_seed(0)
        return models.create_model(name).to(dev).to(memory_format=torch.channels_last).train()

    # ---- the census ----------------------------------------------------------------------------------------------------------------------------------------
    hosts = (models.MetaNeXtBlock, models.Downsample, lsmodels.MetaNeXtBlock, lsmodels.Downsample)
    census = {}                                               # (R, C, dtype of u, epilogue, dtype of r | None) -> {model: calls a step}
    for name in [m for m in args.models.split(",") if m]:
        net = build(name)
        x = torch.randn(args.batch, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
        for amp in (False, True):
            seen, handles = [], []

            def on_norm(epi, slot):
                def hook(mod, inp):
                    u = inp[0]
                    slot.append([u.shape[0] * u.shape[2] * u.shape[3], u.shape[1], u.dtype, epi, None])
                    seen.append(slot[-1])
                return hook

            for m in net.modules():
                if isinstance(m, hosts):
                    seq, slot = m.channel_mixer, []
                    handles.append(seq[0].norm.register_forward_pre_hook(on_norm("gelu", [])))
                    handles.append(seq[2].norm.register_forward_pre_hook(on_norm("add", slot)))
                    handles.append(m.register_forward_hook(lambda mod, inp, out, slot=slot: slot[-1].__setitem__(4, out.dtype)))
                elif isinstance(m, (models.RecNextStem, lsmodels.RecNextStem)):
                    seq = m.stem
                    for i, cn in enumerate(seq):
                        if isinstance(cn, ConvNorm) and i + 1 < len(seq) and isinstance(seq[i + 1], nn.GELU):
                            handles.append(cn.norm.register_forward_pre_hook(on_norm("gelu", [])))
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                net(x)
            for h in handles:
                h.remove()
            for e in seen:
                per = census.setdefault(tuple(e), {})
                per[name] = per.get(name, 0) + 1
        del net, x
        torch.cuda.empty_cache()

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

    def forms(R, c, dt, epi, rdt):
        n = args.batch
        hw = R // n
        h = int(round(hw ** 0.5))
        assert h * h == hw and n * hw == R
        torch.manual_seed(c + h)
        u = (torch.randn(n, h, h, c, device=dev) + 0.3).to(dt).permute(0, 3, 1, 2).requires_grad_(True)
        w = (torch.rand(c, device=dev) + 0.5).requires_grad_(True)
        b = (torch.randn(c, device=dev) * 0.2).requires_grad_(True)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        if epi == "gelu":
            g = torch.randn(n, h, h, c, device=dev).to(dt).permute(0, 3, 1, 2)
            chain = lambda: torch.autograd.grad(F.gelu(F.batch_norm(u, rm, rv, w, b, True, 0.1, 1e-5)), [u, w, b], g)
            fused = lambda: torch.autograd.grad(ops.BnGeluFn.apply(u, w, b, rm, rv, 0.1, 1e-5), [u, w, b], g)
        else:
            r = torch.randn(n, h, h, c, device=dev).to(rdt).permute(0, 3, 1, 2).requires_grad_(True)
            g = torch.randn(n, h, h, c, device=dev).to(rdt).permute(0, 3, 1, 2)
            mask = torch.empty(n, 1, 1, 1, device=dev, dtype=dt).bernoulli_(0.9).div_(0.9)
            scale = mask.float().view(-1)
            chain = lambda: torch.autograd.grad(r + F.batch_norm(u, rm, rv, w, b, True, 0.1, 1e-5) * mask, [u, r, w, b], g)
            fused = lambda: torch.autograd.grad(ops.BnAddFn.apply(u, r, scale, w, b, rm, rv, 0.1, 1e-5), [u, r, w, b], g)
        return {"chain": chain, "fused": fused}

    short = lambda dt: str(dt)[6:] if dt is not None else "-"
    say(f"library_sources_sha256 {source_fingerprint()}")
    say(f"device {torch.cuda.get_device_name(0)}; BatchNorm + GELU and BatchNorm + mask + residual, forward + backward, batch {args.batch}, channels_last; "
        f"{args.rounds} alternating rounds a form; us a call (median of rounds), spread = (max - min) / median; launches a forward + backward: chain 8 and 10, operator 3 + 3")
    say(f"{'epi':>4s} {'C':>4s} {'R':>8s} {'u':>8s} {'r':>8s} | {'chain gpu':>9s} {'spread':>6s} {'fused gpu':>9s} {'spread':>6s} {'ratio':>5s} | "
        f"{'chain wall':>10s} {'spread':>6s} {'fused wall':>10s} {'spread':>6s} {'ratio':>5s} | verdict | calls a step")
    won = {}
    for key in sorted(census, key=lambda k: (k[3], str(k[2]), k[1], k[0], str(k[4]))):
        R, c, dt, epi, rdt = key
        fm = forms(R, c, dt, epi, rdt)
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
        wins = all(ratio[i] > 1.0 + max(spr["chain"][i], args.margin) for i in (0, 1))
        loses = any(ratio[i] < 1.0 - spr["chain"][i] for i in (0, 1))
        verdict = "fused wins" if wins else ("chain wins" if loses else "within the spread")
        rkey = (c, 4 if dt == torch.float32 else 2, epi)
        won.setdefault(rkey, []).append((R, wins))
        say(f"{epi:>4s} {c:4d} {R:8d} {short(dt):>8s} {short(rdt):>8s} | {med['chain'][0]:9.1f} {spr['chain'][0]:6.1%} {med['fused'][0]:9.1f} {spr['fused'][0]:6.1%} {ratio[0]:5.2f} | "
            f"{med['chain'][1]:10.1f} {spr['chain'][1]:6.1%} {med['fused'][1]:10.1f} {spr['fused'][1]:6.1%} {ratio[1]:5.2f} | {verdict} | "
            + ", ".join(f"{m} {k}" for m, k in sorted(census[key].items())))
    table = {k: (min(r for r, w in v if w) // 2, 2 * max(r for r, w in v if w)) for k, v in won.items()
             if any(w for _, w in v) and all(w2 for r2, w2 in v if min(r for r, w in v if w) <= r2 <= max(r for r, w in v if w))}
    say("the table this job alone gives (half the least to twice the largest winning rows of a key, no losing measurement between them): ROUTED = " + repr(table))

    # ---- the step ------------------------------------------------------------------------------------------------------------------------------------------
    def stepper(net):
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
        x = torch.randn(args.batch, 3, 224, 224, device=dev).contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, 1000, (args.batch,), device=dev)

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = F.cross_entropy(net(x).float(), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        return step

    def ms_of(step):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(args.steps):
            step()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / args.steps

    for name in [m for m in args.steps_of.split(",") if m]:
        variants = {"off": build(name), "on (all shapes)": build(name)}
        marked = models.use_fused_mixer_norms_train(variants["on (all shapes)"], all_shapes=True)
        if bnact.ROUTED:
            variants["on (routing rule)"] = build(name)
            models.use_fused_mixer_norms_train(variants["on (routing rule)"])
        steps = {k: stepper(v) for k, v in variants.items()}
        for st in steps.values():
            for _ in range(3):
                st()
        runs = {k: [] for k in steps}
        for _ in range(2):                                    # off / on, twice
            for k, st in steps.items():
                runs[k].append(ms_of(st))
        off = runs["off"]
        spread = abs(off[0] - off[1])
        say(f"step {name} batch {args.batch} bf16 autocast, {marked} modules marked, ms a step ({args.steps} steps a run, off / on alternated twice): "
            + "; ".join(f"{k} {v[0]:.1f} {v[1]:.1f}" for k, v in runs.items()) + f"; the off-runs' spread {spread:.2f} ms")
        for k, v in runs.items():
            if k != "off":
                d = statistics.mean(v) - statistics.mean(off)
                say(f"  {k}: {d:+.2f} ms a step: " + ("resolved" if abs(d) > spread else "not resolved (inside the off-runs' spread)"))
        del variants, steps
        torch.cuda.empty_cache()

    for name in [m for m in args.memory_of.split(",") if m]:
        peak = {}
        for k in ("off", "on"):
            net = build(name)
            if k == "on":
                models.use_fused_mixer_norms_train(net, all_shapes=True)
            st = stepper(net)
            st()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            st()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated()
            del net, st
            torch.cuda.empty_cache()
        say(f"peak torch.cuda.max_memory_allocated of one {name} step, batch {args.batch}, bf16 autocast: off {peak['off'] / 2 ** 20:.0f} MiB, "
            f"on (all shapes) {peak['on'] / 2 ** 20:.0f} MiB, {(peak['on'] - peak['off']) / 2 ** 20:+.0f} MiB")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
