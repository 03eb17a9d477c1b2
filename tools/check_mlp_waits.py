#!/usr/bin/env python3
"""How the hidden-step loops of the channel mixer's ring kernels wait for their LDS reads, from the listing the build keeps (recnext_amd/csrc/_obj/rcx_mlp.s).

Per kernel that calls mlp::hidden_tile_ring / hidden_tile_pinned and per hidden-step loop (the innermost loop with matrix products; k_channel_mlp_stream runs two
hidden steps per iteration), between the loop's first and last product:
    products, ds_reads             per hidden step
    full drains                    s_waitcnt with lgkmcnt(0), per hidden step: each one waits for a request issued right in front of it
    min in flight                  the smallest number of LDS requests any of those waits leaves in flight (0 = a full drain)
A wave's LDS reads return in order, so a product needs lgkmcnt(requests issued behind its fragment's), never 0, until the chain's last fragments.

usage: check_mlp_waits.py [listing.s]        (exit status 0; `--json` prints the rows as one JSON list)"""
import json
import os
import re
import sys

DEFAULT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "recnext_amd", "csrc", "_obj", "rcx_mlp.s")
RING_KERNELS = ("k_channel_mlp_pair", "k_channel_mlp_res128", "k_channel_mlp_stream", "k_channel_mlp")


def functions(lines):
    """(name, first line, last line) of every kernel of the listing"""
    out, name, start = [], None, 0
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z[\w$.]+):", l)
        if m:
            name, start = m.group(1), i
        elif name and l.strip().startswith("s_endpgm"):
            out.append((name, start, i))
            name = None
    return out


def kernel_of(mangled):
    m = re.match(r"_ZN3rcx3mlp(\d+)", mangled)
    if not m:
        return None, []
    n = int(m.group(1))
    rest = mangled[len(m.group(0)):]
    return rest[:n], [int(v) for v in re.findall(r"Li(\d+)E", rest[n:].split("EEv")[0] + "E")]


def step_loops(lines, a, b):
    """innermost backward-branch regions [label line, branch line] of lines a..b that hold matrix products"""
    label = {}
    for i in range(a, b + 1):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
        if m:
            label[m.group(1)] = i
    regions = {}
    for i in range(a, b + 1):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", lines[i])
        if m and m.group(1) in label and label[m.group(1)] < i:
            regions[label[m.group(1)]] = max(regions.get(label[m.group(1)], 0), i)
    regs = [(s, e) for s, e in regions.items() if any("v_mfma" in lines[k] for k in range(s, e + 1))]
    return sorted(r for r in regs if not any(o != r and r[0] <= o[0] <= r[1] for o in regs))      # (a rotated inner loop ends behind its outer loop's branch)


def scan(lines, s, e):
    prods = [k for k in range(s, e + 1) if re.match(r"\s+v_mfma", lines[k])]
    first, last = prods[0], prods[-1]
    reads = drains = flight = 0
    least = None
    for k in range(s, last + 1):
        t = lines[k].strip()
        if re.match(r"ds_(read|write|load|store)", t):
            flight += 1
            if k >= first and t.startswith(("ds_read", "ds_load")):
                reads += 1
        m = re.match(r"s_waitcnt\b.*lgkmcnt\((\d+)\)", t)
        if m:
            n = int(m.group(1))
            if k > first:
                drains += n == 0
                left = min(flight, n)
                least = left if least is None else min(least, left)
            flight = min(flight, n)
    # the reads in front of the first product (the ring's preload) belong to the step
    reads += sum(1 for k in range(s, first) if lines[k].strip().startswith(("ds_read", "ds_load")))
    return len(prods), reads, drains, least


def report(path):
    lines = open(path).read().split("\n")
    rows = []
    for name, a, b in functions(lines):
        kern, targs = kernel_of(name)
        if kern not in RING_KERNELS or len(targs) < 3:
            continue
        ks1, ct = targs[0], targs[2]
        for s, e in step_loops(lines, a, b):
            prods, reads, drains, least = scan(lines, s, e)
            steps = max(1, round(prods / (ks1 + 2 * ct)))
            rows.append({"kernel": kern, "template": targs, "loop_line": s + 1, "steps_per_iteration": steps, "products_per_step": prods / steps, "ds_reads_per_step": reads / steps,
                         "full_drains_per_step": drains / steps, "min_in_flight": least})
    return rows


def main():
    args = [v for v in sys.argv[1:] if not v.startswith("--")]
    rows = report(args[0] if args else DEFAULT)
    if "--json" in sys.argv:
        print(json.dumps(rows))
        return
    print(f"{'kernel':22s} {'template arguments':28s} {'loop at':>8s} {'products':>9s} {'ds_reads':>9s} {'full drains':>12s} {'min in flight':>14s}   (per hidden step)")
    for r in rows:
        print(f"{r['kernel']:22s} {','.join(map(str, r['template'])):28s} {r['loop_line']:8d} {r['products_per_step']:9.1f} {r['ds_reads_per_step']:9.1f} "
              f"{r['full_drains_per_step']:12.1f} {str(r['min_in_flight']):>14s}")


if __name__ == "__main__":
    main()
