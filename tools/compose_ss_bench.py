#!/usr/bin/env python3
"""Times supersampled compose against compose at equal sample count: six 1024^2 RGBA cube faces,
bicubic, FIRST or FEATHER, about 8.4 M samples per launch in every row —

  n = 1   lrp_compose_device into 4096 x 2048 (the yardstick: the kernel of DESIGN.md section 12);
  n = 2   lrp_compose_ss_device into 2048 x 1024;
  n = 3   lrp_compose_ss_device into 1365 x 683;
  n = 4   lrp_compose_ss_device into 1024 x 512.

One row per process; alternate them in rounds.

usage: compose_ss_bench.py 1|2|3|4 first|feather [--root DIR] [--face N] [--interp I] [--shrink K] [--reps R] [--warmup W]
--root: the checkout whose package is measured (default: this one); --face, --interp: another face size or sampler; --shrink K:
the output K times smaller again at the same n (neighbouring lanes K times further apart in the sources: --face 2048 --shrink 2
at n = 1 takes the yardstick's 8.4 M samples the way the n = 2 row's lanes are spaced) — to see what a difference between the
rows follows.  Prints one line: average and minimum us per iteration
(events around every iteration), samples per second and the checksum of the result."""
import argparse
import importlib
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int, choices=[1, 2, 3, 4])
    ap.add_argument("mode", choices=["first", "feather"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--face", type=int, default=1024)
    ap.add_argument("--interp", type=int, default=2, choices=[0, 1, 2])
    ap.add_argument("--shrink", type=int, default=1)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch

    lrp = importlib.import_module("image-lens-reproject_amd")
    f, n, C = a.face, a.n, 4
    ow, oh = round(4 * f / (n * a.shrink)), round(2 * f / (n * a.shrink))  # (n = 3: 1365 x 683)
    d2r = np.float32(np.pi / 180.0)
    angles = [(0, 0), (90, 0), (180, 0), (270, 0), (0, 90), (0, -90)]  # pan, pitch of the six faces
    rots = [lrp.rotation_matrix(float(np.float32(p) * d2r), float(np.float32(t) * d2r), 0.0) for p, t in angles]
    face_lens, pano = lrp.LensInfo.rectilinear(18.0, 36.0, f, f), lrp.LensInfo.equirectangular()
    srcs = []
    for i in range(6):
        t = torch.empty((f, f, C), dtype=torch.float32, device="cuda")
        lrp.synth_fill(t, f, f, C, 0xC0B0 + i)
        srcs.append(t)
    ins = [lrp.Image(face_lens, f, f, C, t) for t in srcs]
    out = torch.empty((oh, ow, C), dtype=torch.float32, device="cuda")
    out_image = lrp.Image(pano, ow, oh, C, out)
    mode = 2 if a.mode == "feather" else 0

    if n == 1:
        def run():
            lrp.compose(ins, out_image, a.interp, rots, mode)
    else:
        def run():
            lrp.compose_ss(ins, out_image, n, a.interp, rots, mode)

    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    what = "compose" if n == 1 else "compose_ss"
    print(f"cube6x{f}_eqr_{('nn', 'bl', 'bc')[a.interp]} {what:10s} n {n} {ow:4d}x{oh:<4d} {a.mode:7s} avg {np.mean(times):9.1f} us  min {np.min(times):9.1f} us  "
          f"{ow * oh * n * n / np.mean(times) / 1e3:7.2f} Gsamples/s  checksum {lrp.checksums([out])[0]:016x}", flush=True)


if __name__ == "__main__":
    main()
