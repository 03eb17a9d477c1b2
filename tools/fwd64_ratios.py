#!/usr/bin/env python3
"""The worst err / (2**-24 * M) per operator, kernel and I/O type out of the junit report of tests/test_forward_f64_gpu.py
(pytest tests/test_forward_f64_gpu.py -m gpu --junitxml=REPORT -o junit_family=xunit1): the table of profiles/r22_forward_f64_ratios.txt.

usage: fwd64_ratios.py REPORT.xml"""
import ast
import collections
import re
import sys
import xml.etree.ElementTree as ET

TYPES = ("f32", "bf16", "f16")


def main(path):
    worst = collections.defaultdict(lambda: collections.defaultdict(float))          # (operator, kernel) -> output type -> ratio
    count = collections.Counter()
    for tc in ET.parse(path).getroot().iter("testcase"):
        props = {p.get("name"): p.get("value") for p in tc.iter("property")}
        if "ratios" not in props or not tc.get("classname", "").endswith("test_forward_f64_gpu"):
            continue
        op = re.match(r"test_(\w+?)(?:_forward)?_matches_float64", tc.get("name")).group(1)
        for key, (r, n) in ast.literal_eval(props["ratios"]).items():                  # "kernel outtype" -> (worst ratio, checks)
            kern, out = key.rsplit(" ", 1)
            worst[(op, kern)][out] = max(worst[(op, kern)][out], r)
            count[(op, kern)] += n
    print(f"{'operator':<16}{'kernel / schedule family':<28}{'checks':>7}" + "".join(f"{t:>8}" for t in TYPES))
    for (op, kern), by in sorted(worst.items()):
        print(f"{op:<16}{kern:<28}{count[(op, kern)]:>7}" + "".join(f"{by[t]:>8.2f}" if t in by else f"{'-':>8}" for t in TYPES))
    print(f"worst over all: {max(max(by.values()) for by in worst.values()):.2f}")


if __name__ == "__main__":
    main(sys.argv[1])
