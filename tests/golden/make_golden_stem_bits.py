#!/usr/bin/env python3
"""Record tests/golden/stem_parent_bits.json: per case of tests/test_stem_pipeline_gpu.py, the seed of its CPU generator and the sha256 of the bytes the stem wrote.

RUN THIS ON THE PARENT'S BUILD ONLY, on the GPU, BEFORE any change to k_stem: commit c7ce1f4 ("Hold every linear forward kernel to float64 with per-element
bounds"), the last one whose rcx_stem.hip runs a wave's pixel tiles one after the other.  The file is the record of what that kernel computed; the test asserts
that the pipelined kernel writes the same bits.  Recording it from a later build would make the test compare the kernel with itself.

    python tests/golden/make_golden_stem_bits.py [OUT.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import test_stem_pipeline_gpu as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    rec = {}
    for name, case in t.CASES.items():
        launch, _ = t.make_case(name)
        y = launch()
        assert torch.equal(launch(), y)
        rec[name] = {"seed": case[-1], "sha256": t.output_sha256(y)}
        print(name, rec[name]["sha256"])
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
