#!/usr/bin/env python3
"""Times one 4096^2 RGBA float frame through lrp_reproject_device under the Lanczos-3 sampler, or under the bicubic sampler as a
yardstick, one figure per process:

usage: lanczos_bench.py lanczos|bicubic GEOMETRY [--root DIR] [--family F] [--first] [--size N] [--reps R] [--warmup W]
       lanczos_bench.py rounds [--root PARENT_CHECKOUT] [--rounds 4] [--size N]
GEOMETRY: c1   BASELINE configs[1]: fisheye (180 degrees) -> rectilinear, no rotation
          c2   configs[2]: panorama -> fisheye, rotated
--root: the checkout whose package is measured (default: this one; `bicubic` on the parent commit's library is the yardstick).
--family: lrp_debug_kernel(F) for `bicubic`: 0 is the one-pixel-per-lane kernel (the shape of the Lanczos kernels, 16 taps), the
default (-1) leaves the planner's choice.
--first: every timed iteration is a first call — the lens tables and the geometry cache are released before it, outside the timed
interval; otherwise the launches read the geometry-cache entry the warm-up wrote.
`rounds` is the driver: per round one process per figure, alternating; it ends with the mean of the rounds' means and their
minimum - maximum per figure.  Timing: device events around every iteration."""
import argparse
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np

GENERAL = (30.0, -15.0, 5.0)
GEOMETRIES = {"c1": dict(inp="eqd", out="rect", deg=None), "c2": dict(inp="eqr", out="eqd", deg=GENERAL)}


def rounds(argv):
    """The driver: fresh processes (this one never opens the GPU), alternating within a round; a failed one ends the run."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="the parent commit's checkout, built (default: this one)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args(argv)
    me = os.path.abspath(__file__)
    here = os.path.dirname(os.path.dirname(me))
    parent = a.root or here
    plan = []
    for g in ("c1", "c2"):
        plan.append((f"{g} lanczos cache read", ["lanczos", g, "--root", here]))
        plan.append((f"{g} lanczos first call", ["lanczos", g, "--root", here, "--first", "--reps", "10", "--warmup", "2"]))
        plan.append((f"{g} parent bicubic, family 0", ["bicubic", g, "--root", parent, "--family", "0"]))
        plan.append((f"{g} parent bicubic, default", ["bicubic", g, "--root", parent]))
    means = {k: [] for k, _ in plan}
    for r in range(a.rounds):
        print(f"-- round {r + 1}", flush=True)
        for key, args in plan:
            p = subprocess.run([sys.executable, me] + args + ["--size", str(a.size)], capture_output=True, text=True, timeout=300)
            sys.stdout.write(p.stdout)
            sys.stdout.flush()
            if p.returncode != 0:
                sys.stderr.write(p.stderr)
                return p.returncode
            means[key].append(float(re.search(r"mean\s+([0-9.]+) us", p.stdout).group(1)))
    print("-- mean of the rounds' means, minimum - maximum of them (us)")
    for key, _ in plan:
        v = means[key]
        print(f"{key:30s} {np.mean(v):9.1f}  {np.min(v):9.1f} - {np.max(v):9.1f}", flush=True)
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rounds":
        sys.exit(rounds(sys.argv[2:]))
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["lanczos", "bicubic"])
    ap.add_argument("geometry", choices=sorted(GEOMETRIES))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--family", type=int, default=-1)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--first", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch

    lrp = importlib.import_module("image-lens-reproject_amd")
    geo, n, C = GEOMETRIES[a.geometry], a.size, 4

    def lens(kind):
        L = lrp.LensInfo
        return {"rect": L.rectilinear(18.0, 36.0, n, n), "eqd": L.equidistant(math.pi), "eqr": L.equirectangular()}[kind]

    lin, lout = lens(geo["inp"]), lens(geo["out"])
    rot = None
    if geo["deg"] is not None:
        rot = lrp.rotation_matrix(*[float(np.float32(d) * np.float32(math.pi) / np.float32(180.0)) for d in geo["deg"]])
    gen = torch.Generator(device="cuda").manual_seed(5)
    d_in = torch.rand((n, n, C), device="cuda", generator=gen)
    d_out = torch.zeros((n, n, C), dtype=torch.float32, device="cuda")
    im_in, im_out = lrp.Image(lin, n, n, C, d_in), lrp.Image(lout, n, n, C, d_out)
    lrp.geometry_cache_configure(-1, 1)  # (an entry on the first sighting of a geometry)
    if a.what == "lanczos":
        lrp.sampler_extensions(lrp.SAMPLER_EXT_LANCZOS3)
        interp, label = lrp.LANCZOS3, "lanczos"
    else:
        if a.family >= 0:
            lrp.debug_kernel(a.family)
        interp, label = 2, "bicubic " + (f"family {a.family}" if a.family >= 0 else "default ")

    def run():
        lrp.reproject(im_in, im_out, 1, interp, rot)

    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        if a.first:
            torch.cuda.synchronize()
            lrp.release_cached_tables()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    stats = lrp.geometry_cache_stats()
    checksum = lrp.checksums([d_out])[0]
    print(f"{a.geometry} {n}^2 {label:18s} {'first call' if a.first else 'cache read'} mean {np.mean(times):9.1f} us  "
          f"min - max {np.min(times):9.1f} - {np.max(times):9.1f} us  {n * n / np.mean(times) / 1e3:7.2f} Gpix/s  "
          f"fills {stats['fills']} hits {stats['hits']}  checksum {checksum:016x}", flush=True)


if __name__ == "__main__":
    main()
