#!/usr/bin/env python3
"""Times a packed frame through the device in one of two ways, one per process:

  fused   one lrp_reproject_packed_device launch;
  chain   the calls that existed before it: decode_pixels, reproject (lrp_reproject_device), encode_pixels, with the two
          float32 staging images allocated beforehand.

usage: packed_bench.py fused|chain ROW [--root DIR] [--size N] [--reps R] [--warmup W] [--first] [--cache 0|1]
       packed_bench.py rounds [--root PARENT_CHECKOUT] [--rounds 4] [--size N]
`rounds` is the driver: per round and row one process each, alternating, for the yardstick (`chain` on the library of --root, the
parent commit's checkout) and for `fused` on this checkout, a cache-reading launch and a first call; then, for the geometries
the planner exempts from the coordinate map, `fused --cache 1` against `fused --cache 0`.  It ends with the mean of the rounds'
means and their minimum - maximum per figure.
ROW: c1_rgba8       BASELINE configs[1], fisheye -> rect bicubic, RGBA8 -> RGBA8
     c2_rgba8       configs[2], equirect -> fisheye bilinear rotated, RGBA8 -> RGBA8
     c1_half_post   configs[1], RGBA half + tonemap -> RGBA8
     nn_norot       equirect -> rect nearest, no rotation            } the geometries the planner of lrp_reproject_device exempts
     rect_rect_bl   rectilinear -> rectilinear bilinear, rotated     } from the coordinate map: time --cache 1 against --cache 0
     rect_pano_nn   rectilinear -> panorama nearest                  }
--root: the checkout whose package is measured (default: this one; `chain` on the parent commit's library is the yardstick).
--first: every timed iteration is a first call — the lens tables and the geometry cache are released before it, outside the
timed interval (the 8-bit conversion tables, which the release drops too, are uploaded again by a one-pixel decode, also
outside it: a process converts its first pixel once, not once per geometry).  --cache 0: lrp_debug_set("geo_cache", 0), every
launch computes its coordinates.
Prints one line: mean and minimum - maximum us per iteration (events around every iteration), the device bytes the approach holds
(packed frames, staging images, the geometry-cache entry) and a checksum of the output bytes."""
import argparse
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np

F32, F16, U8 = 0, 1, 2
GENERAL = (30.0, -15.0, 5.0)
ROWS = {
    "c1_rgba8": dict(inp="eqd", out="rect", interp=2, deg=None, in_fmt=U8, out_fmt=U8, post=None),
    "c2_rgba8": dict(inp="eqr", out="eqd", interp=1, deg=GENERAL, in_fmt=U8, out_fmt=U8, post=None),
    "c1_half_post": dict(inp="eqd", out="rect", interp=2, deg=None, in_fmt=F16, out_fmt=U8, post=(2.0, 4.0)),
    "nn_norot": dict(inp="eqr", out="rect", interp=0, deg=None, in_fmt=U8, out_fmt=U8, post=None),
    "rect_rect_bl": dict(inp="rect", out="rect", interp=1, deg=GENERAL, in_fmt=U8, out_fmt=U8, post=None),
    "rect_pano_nn": dict(inp="rect", out="eqr", interp=0, deg=None, in_fmt=U8, out_fmt=U8, post=None),
}


def rounds(argv):
    """The driver: fresh processes (this one never opens the GPU), alternating within a round; a failed one ends the run."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=None, help="the parent commit's checkout, built (default: this one, i.e. no yardstick of its own)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--size", type=int, default=4096)
    a = ap.parse_args(argv)
    me = os.path.abspath(__file__)
    here = os.path.dirname(os.path.dirname(me))
    plan = []
    for row in ("c1_rgba8", "c2_rgba8", "c1_half_post"):
        for first in (False, True):
            extra = ["--first", "--reps", "10", "--warmup", "2"] if first else []
            plan.append((f"{row} {'first' if first else 'read '} chain", ["chain", row, "--root", a.root or here] + extra))
            plan.append((f"{row} {'first' if first else 'read '} fused", ["fused", row, "--root", here] + extra))
    for row in ("nn_norot", "rect_rect_bl", "rect_pano_nn"):
        for cache in (1, 0):
            plan.append((f"{row} fused cache {cache}", ["fused", row, "--root", here, "--cache", str(cache)]))
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
        print(f"{key:28s} {np.mean(v):9.1f}  {np.min(v):9.1f} - {np.max(v):9.1f}", flush=True)
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "rounds":
        sys.exit(rounds(sys.argv[2:]))
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["fused", "chain"])
    ap.add_argument("row", choices=sorted(ROWS))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--first", action="store_true")
    ap.add_argument("--cache", type=int, default=1)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch

    lrp = importlib.import_module("image-lens-reproject_amd")
    row, n, C = ROWS[a.row], a.size, 4

    def lens(kind):
        L = lrp.LensInfo
        return {"rect": L.rectilinear(18.0, 36.0, n, n), "eqd": L.equidistant(math.pi), "eqr": L.equirectangular()}[kind]

    lin, lout = lens(row["inp"]), lens(row["out"])
    rot = None
    if row["deg"] is not None:
        rot = lrp.rotation_matrix(*[float(np.float32(d) * np.float32(math.pi) / np.float32(180.0)) for d in row["deg"]])
    gen = torch.Generator(device="cuda").manual_seed(5)
    if row["in_fmt"] == U8:
        d_in = torch.randint(0, 256, (n, n, C), dtype=torch.uint8, device="cuda", generator=gen)
    else:
        d_in = (torch.rand((n, n, C), device="cuda", generator=gen) * 2).to(torch.float16).view(torch.int16)
    d_out = torch.zeros((n, n, C), dtype={U8: torch.uint8, F16: torch.int16, F32: torch.float32}[row["out_fmt"]], device="cuda")
    held = d_in.numel() * d_in.element_size() + d_out.numel() * d_out.element_size()
    lrp.debug_set("geo_cache", a.cache)
    lrp.geometry_cache_configure(-1, 1)  # (an entry on the first sighting of a geometry)

    if a.what == "fused":
        im_in, im_out = lrp.Image(lin, n, n, C, None), lrp.Image(lout, n, n, C, None)

        def run():
            lrp.reproject_packed(im_in, row["in_fmt"], d_in, im_out, row["out_fmt"], d_out, 255, 1, row["interp"], rot, post=row["post"])
    else:
        tmp_in = torch.empty((n, n, C), dtype=torch.float32, device="cuda")
        tmp_out = torch.empty((n, n, C), dtype=torch.float32, device="cuda")
        held += 2 * tmp_in.numel() * 4
        im_in, im_out = lrp.Image(lin, n, n, C, tmp_in), lrp.Image(lout, n, n, C, tmp_out)

        def run():
            lrp.decode_pixels(d_in, row["in_fmt"], tmp_in)
            lrp.reproject(im_in, im_out, 1, row["interp"], rot, post=row["post"])
            lrp.encode_pixels(tmp_out, d_out, row["out_fmt"], fill=255)

    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    entry = lrp.geometry_cache_stats()["bytes"]
    one_in, one_f = torch.zeros((1, 1, 4), dtype=torch.uint8, device="cuda"), torch.zeros((1, 1, 4), dtype=torch.float32, device="cuda")
    times = []
    for _ in range(a.reps):
        if a.first:
            torch.cuda.synchronize()
            lrp.release_cached_tables()
            lrp.decode_pixels(one_in, U8, one_f)  # (the 8-bit tables again)
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    checksum = int(d_out.view(torch.uint8).to(torch.int64).sum().item())
    print(f"{a.row:13s} {n}^2 {a.what:5s} {'first call' if a.first else 'cache ' + ('read' if a.cache else 'off '):10s} "
          f"mean {np.mean(times):9.1f} us  min - max {np.min(times):9.1f} - {np.max(times):9.1f} us  {n * n / np.mean(times) / 1e3:7.2f} Gpix/s  "
          f"held {(held + entry) / 2 ** 20:7.1f} MiB (entry {entry / 2 ** 20:.1f})  sum {checksum}", flush=True)


if __name__ == "__main__":
    main()
