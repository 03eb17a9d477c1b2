"""The share block's token half (recnext_amd.lsshare.ls_share, one launch) against the three-launch chain it replaces (ops.dwconv2d + torch.cat +
add), bf16, at the share-channel RecNeXt-T / S / B's own shape and at the 7 x 7 plane.  Run each form under a kernel trace of its own and sum:

    rocprofv3 --kernel-trace --output-format csv -d OUT/share -- python tools/bench_ls_share.py share
    rocprofv3 --kernel-trace --output-format csv -d OUT/chain -- python tools/bench_ls_share.py chain
    python tools/bench_ls_share.py sum OUT/share        # calls, total and mean microseconds per kernel name and grid

(profiles/r14_ls_share.txt)."""
import collections
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(256, 512, 4, 4), (256, 512, 7, 7)]
ITERS = 320


def run(which):
    import torch
    from recnext_amd import lsshare, ops
    dev = torch.device("cuda:0")
    for (b, c, h, w) in SHAPES:
        torch.manual_seed(0)
        blk = lsshare.ShareBlock(c, 1.5).eval().to(dev).requires_grad_(False)
        mk = lambda: torch.randn(b, c, h, w, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
        x = mk()
        srcs = [mk()[:, :c // 4] for _ in range(4)]              # t_prev[:, :split] of four earlier token halves
        wr, br = blk.packed_params()
        with torch.no_grad():
            for _ in range(ITERS):
                if which == "share":
                    r, t = lsshare.ls_share(x, wr, br, srcs)
                else:
                    r = ops.dwconv2d(x, wr, br, k=3, stride=1)
                    t = r + torch.cat(srcs, dim=1)
            torch.cuda.synchronize()
    print("done", which, ITERS, "iterations per shape")


def summarise(directory):
    tot = collections.defaultdict(lambda: [0, 0.0])
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            key = row["Kernel_Name"][:110] + " grid=" + row.get("Grid_Size_X", "?")
            tot[key][0] += 1
            tot[key][1] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
    for key, (n, us) in sorted(tot.items(), key=lambda kv: -kv[1][1]):
        print(f"{n:6d} calls {us:12.1f} us total {us / n:9.2f} us/call  {key}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "sum":
        summarise(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] in ("share", "chain"):
        run(sys.argv[1])
    else:
        raise SystemExit(__doc__)
