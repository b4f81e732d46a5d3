#!/usr/bin/env python3
"""Regenerates tests/golden/coverage_golden.json: the digest of the CPU model's coverage plane (tests/coverage_model.py) for the
full frame of tests/coverage_cases.py — the BASELINE configs[3] geometry at 4096 x 4096.  tests/test_gpu_coverage.py compares the
HIP plane with the committed value and calls no model at that size; tests/test_coverage.py renders it again on the CPU.

Run from the repo root after __graft_entry__.build() (a few seconds):
    python tests/golden/make_coverage_golden.py
"""
import hashlib
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import coverage_cases as cc  # noqa: E402
import coverage_model as model  # noqa: E402

lrp = importlib.import_module("image-lens-reproject_amd")
OUT = os.path.join(HERE, "coverage_golden.json")


def digest(case):
    (iw, ih), (ow, oh), n = case["in_size"], case["out_size"], case["n"]
    plane = model.coverage(cc.lens(lrp, case["inp"], iw, ih), iw, ih, cc.lens(lrp, case["out"], ow, oh), ow, oh, n, cases.rotation(lrp, case["deg"]))
    return dict(case={k: (list(v) if isinstance(v, tuple) else v) for k, v in case.items()}, sha256=hashlib.sha256(plane.tobytes()).hexdigest(),
                count0=int((plane == 0).sum()), count_full=int((plane == n * n).sum()))


def main():
    frame = digest(cc.FULL_FRAME)
    print(f"{frame['case']['name']}: {frame['sha256'][:16]} count 0 {frame['count0']}, count n*n {frame['count_full']}")
    with open(OUT, "w") as f:
        json.dump(dict(generator="tests/golden/make_coverage_golden.py", frame=frame), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
