#!/usr/bin/env python3
"""Regenerates tests/golden/stereographic_golden.json: whole-frame digests of the CPU model's output
(tests/stereographic_model.py, the oracle's loop with the stereographic lens extension) for the cases of
tests/stereographic_cases.py.  tests/test_gpu_stereographic_golden.py compares the HIP output with these committed values and
calls no model on the GPU box.

Run from the repo root after __graft_entry__.build() (a few minutes on 8 cores):
    python tests/golden/make_stereographic_golden.py
"""
import importlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import fullframe_cases as ffc  # noqa: E402
import oracle_binding as oracle  # noqa: E402
import stereographic_cases as stc  # noqa: E402
import stereographic_model as model  # noqa: E402

lrp = importlib.import_module("image-lens-reproject_amd")
OUT = os.path.join(HERE, "stereographic_golden.json")
THREADS = max(1, len(os.sched_getaffinity(0)))


def render(case):
    (iw, ih), (ow, oh), c = case["in_size"], case["out_size"], case["c"]
    src = oracle.synth_frame(iw, ih, c, case["seed"], depth_channel=case["depth"])
    lin, lout = stc.lens(lrp, case["inp"], iw, ih), stc.lens(lrp, case["out"], ow, oh)
    return model.reproject(lin, src, lout, ow, oh, 1, case["interp"], cases.rotation(lrp, case["deg"]), post=case["post"], threads=THREADS)


def main():
    frames = {}
    for name, case in sorted(stc.frame_cases().items()):
        t = time.time()
        sha, bands, n_nan = ffc.frame_digests(render(case))
        frames[name] = dict(case={k: (list(v) if isinstance(v, tuple) else v) for k, v in case.items() if k != "name"},
                            sha256=sha, bands=bands, nan=n_nan)
        print(f"{name}: {sha[:16]} nan {n_nan} ({time.time() - t:.1f} s)", flush=True)
    with open(OUT, "w") as f:
        json.dump(dict(generator="tests/golden/make_stereographic_golden.py", frames=frames), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
