"""Inference throughput of the LSNet-style RecNeXt-T / S / B across input sizes, in one process: the HIP token half (one-workgroup entries where
they apply, the tiled entries elsewhere) against (a) the dispatch before the tiled entries existed -- their support queries masked, so the
library chain or NotImplementedError comes back -- and (b) the same model with the token half on the operator chain of tests/ls_eager.py.
The three paths of a (model, size) run back to back, so they share the box's state.  A path that raises is recorded with its error and the
sweep goes on.  One JSON line per (model, size, path), each with library_sources_sha256.

    python tools/bench_ls_resolutions.py [--models recnext_t,recnext_s,recnext_b] [--sizes 224,256,384,512] [--batch-size 64] [--dtype bf16]
                                         [--t0 1] [--t1 2] [--out profiles/r11_ls_resolutions.jsonl]
    python tools/bench_ls_resolutions.py --models recnext_s --sizes 384 --once      # one forward after a warm-up (for a kernel trace)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from recnext_amd import lsmodels, ops, speed  # noqa: E402
from recnext_amd.build import source_fingerprint  # noqa: E402
from tests.ls_eager import eager_token_mixer  # noqa: E402

PATHS = (("hip", None, False), ("hip_without_tiled", None, True), ("ops_chain", eager_token_mixer, False))


class _masked_tiled_queries:
    """The dispatch of MetaNeXtBlock.token_half before the tiled entries: both tiled support queries answer no."""

    def __enter__(self):
        self.real = (ops.ls_recattn_tiled_supported, ops.ls_la3_tiled_supported)
        ops.ls_recattn_tiled_supported = ops.ls_la3_tiled_supported = lambda *a, **kw: False

    def __exit__(self, *exc):
        ops.ls_recattn_tiled_supported, ops.ls_la3_tiled_supported = self.real


def tiled_blocks(name, size, dtype):
    """(blocks on a tiled entry, blocks in all) of one forward."""
    tiled = total = 0
    for (_, h, w, c, s, heads, kind, blocks) in lsmodels.mixer_shapes(name, size):
        one = (ops.ls_la3_supported if kind == "la3" else ops.ls_recattn_supported)(1, h, w, c, s, heads, dtype)
        tiled, total = tiled + (0 if one else blocks), total + blocks
    return tiled, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="recnext_t,recnext_s,recnext_b")
    ap.add_argument("--sizes", default="224,256,384,512")
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=sorted(speed.DTYPES))
    ap.add_argument("--t0", type=float, default=1.0)
    ap.add_argument("--t1", type=float, default=2.0)
    ap.add_argument("--once", action="store_true", help="HIP path only: warm up, then one synchronised forward")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dtype = speed.DTYPES[args.dtype]
    dev = "cuda:0"
    sha = source_fingerprint()
    out = open(args.out, "w") if args.out else None
    for name in args.models.split(","):
        for size in (int(v) for v in args.sizes.split(",")):
            tiled, total = tiled_blocks(name, size, dtype)
            for path, mixer, masked in (PATHS[:1] if args.once else PATHS):
                rec = dict(model=name, resolution=size, token_half=path, batch_size=args.batch_size, dtype=args.dtype, tiled_blocks=tiled, blocks=total,
                           device=torch.cuda.get_device_name(0), library_sources_sha256=sha)
                try:
                    net = speed.build_inference_model(name, dev, dtype, token_mixer=mixer)
                    with torch.no_grad(), (_masked_tiled_queries() if masked else torch.no_grad()):
                        if args.once:
                            x = speed.synthetic_batch(args.batch_size, size, dev, dtype)
                            for _ in range(3):
                                net(x)
                            torch.cuda.synchronize()
                            net(x)
                            torch.cuda.synchronize()
                            continue
                        rec["images_per_s"] = round(speed.throughput(name, net, dev, args.batch_size, size, dtype, args.t0, args.t1, quiet=True), 1)
                except (NotImplementedError, ValueError) as e:            # no kernel for a shape on this path: a result, not a failure of the sweep
                    rec["error"] = f"{type(e).__name__}: {e}"[:200]
                print(json.dumps(rec), flush=True)
                if out:
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
                net = None
                torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
