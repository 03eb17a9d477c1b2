"""Throughput of the LSNet-style RecNeXt-T / S / B: the HIP token half against the same models with the token half on the operator chain of
tests/ls_eager.py, in one process (recnext_amd.speed's loop: BN folded, channels_last, tuned GEMMs).  One JSON line per (model, path).

    python tools/ls_speed.py [--models recnext_t,recnext_s,recnext_b] [--batch-size 256] [--dtype bf16] [--t0 3] [--t1 6] [--paths hip,ops_chain] [--out FILE]
    python tools/ls_speed.py --models recnext_t --batch-size 256 --once      # one forward after a warm-up (for a kernel trace)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from recnext_amd import speed  # noqa: E402
from recnext_amd.build import source_fingerprint  # noqa: E402
from tests.ls_eager import eager_token_mixer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="recnext_t,recnext_s,recnext_b")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--resolution", type=int, default=224)
    ap.add_argument("--dtype", default="bf16", choices=sorted(speed.DTYPES))
    ap.add_argument("--t0", type=float, default=3.0)
    ap.add_argument("--t1", type=float, default=6.0)
    ap.add_argument("--once", action="store_true", help="HIP path only: warm up, then one synchronised forward")
    ap.add_argument("--paths", default="hip,ops_chain", help="which token halves to time: hip, ops_chain or both")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not args.paths or set(args.paths.split(",")) - {"hip", "ops_chain"}:
        ap.error(f"--paths takes hip, ops_chain or both, got {args.paths!r}")
    dtype = speed.DTYPES[args.dtype]
    dev = "cuda:0"
    lines = []
    for name in args.models.split(","):
        paths = (("hip", None),) if args.once else tuple(p for p in (("hip", None), ("ops_chain", eager_token_mixer)) if p[0] in args.paths.split(","))
        for path, mixer in paths:
            net = speed.build_inference_model(name, dev, dtype, token_mixer=mixer)
            with torch.no_grad():
                if args.once:
                    x = speed.synthetic_batch(args.batch_size, args.resolution, dev, dtype)
                    for _ in range(3):
                        net(x)
                    torch.cuda.synchronize()
                    net(x)
                    torch.cuda.synchronize()
                    continue
                rate = speed.throughput(name, net, dev, args.batch_size, args.resolution, dtype, args.t0, args.t1, quiet=True)
            rec = dict(model=name, token_half=path, images_per_s=rate, batch_size=args.batch_size, resolution=args.resolution, dtype=args.dtype,
                       device=torch.cuda.get_device_name(0), library_sources_sha256=source_fingerprint())
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del net
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
