#!/usr/bin/env python3
"""Times exposure matching across a camera rig on the rig of tools/camera_bench.py row a: six 2048^2 BROWN
cameras (a cube's faces with the barrel distortion of a wide lens), RGBA, into an equirectangular output of 4096 x 2048 or
1024 x 512 —

  stat    the overlap statistic by one launch: lrp_camera_overlap_device;
  hand    the same table by hand: six one-camera lrp_compose_cameras_device renders (bilinear, n = 1, a coverage plane each)
          plus the masked sums in torch (the 36 entries the rig can have);
  plain   lrp_compose_cameras_device (--interp, --mode, n);
  gain    lrp_compose_cameras_gain_device on the same scene, with gains 0.8 .. 1.3.

One row per process; alternate them in rounds.

usage: camera_gain_bench.py stat|hand|plain|gain [--size 4096x2048|1024x512] [--n 1|2] [--interp I] [--mode first|mean|feather]
                            [--root DIR] [--reps R] [--warmup W]
--root: the checkout whose package is measured (default: this one; `hand` and `plain` run on a checkout without the feature too).
Prints one line: average, median and minimum us per repetition (events around every repetition) and a checksum — of the table for
stat and hand, which must agree, of the image otherwise."""
import argparse
import importlib
import os
import sys

import numpy as np

BROWN_K = (-0.12, 0.03, 0.0005, -0.0003, -0.004)  # tools/camera_bench.py row a
LO, HI = 0.02, 0.98


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=["stat", "hand", "plain", "gain"])
    ap.add_argument("--size", default="4096x2048", choices=["4096x2048", "1024x512"])
    ap.add_argument("--n", type=int, default=1, choices=[1, 2])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--interp", type=int, default=2, choices=[0, 1, 2])
    ap.add_argument("--mode", default="feather", choices=["first", "mean", "feather"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch

    lrp = importlib.import_module("image-lens-reproject_amd")
    C, f = 4, 2048
    ow, oh = (int(v) for v in a.size.split("x"))
    d2r = np.float32(np.pi / 180.0)
    angles = [(0, 0), (90, 0), (180, 0), (270, 0), (0, 90), (0, -90)]  # pan, pitch
    rots = [lrp.rotation_matrix(float(np.float32(p) * d2r), float(np.float32(t) * d2r), 0.0) for p, t in angles]
    srcs = []
    for i in range(6):
        t = torch.empty((f, f, C), dtype=torch.float32, device="cuda")
        lrp.synth_fill(t, f, f, C, 0xCA00 + i)
        srcs.append(t)
    centre = f / 2 - 0.5
    cams = [lrp.Camera.brown(f, f, t, f / 2.0, f / 2.0, centre, centre, BROWN_K) for t in srcs]
    pano = lrp.LensInfo.equirectangular()
    out = torch.empty((oh, ow, C), dtype=torch.float32, device="cuda")
    out_image = lrp.Image(pano, ow, oh, C, out)
    mode = {"first": 0, "mean": 1, "feather": 2}[a.mode]
    gains = np.linspace(0.8, 1.3, 6).astype(np.float32)

    if a.row == "stat":
        stats = torch.empty((8, 8, 2), dtype=torch.int64, device="cuda")

        def run():
            lrp.camera_overlap(cams, out_image, rots, LO, HI, stats=stats)
            return stats
    elif a.row == "hand":
        frames = [torch.empty((oh, ow, C), dtype=torch.float32, device="cuda") for _ in cams]
        planes = [torch.empty((oh, ow), dtype=torch.uint8, device="cuda") for _ in cams]
        stats = torch.zeros((8, 8, 2), dtype=torch.int64, device="cuda")

        def run():
            valid, q = [], []
            for cam, rot, frame, plane in zip(cams, rots, frames, planes):
                lrp.compose_cameras([cam], lrp.Image(pano, ow, oh, C, frame), 1, 1, [rot], 0, coverage=plane)
                Y = (0.25 * frame[..., 0] + 0.5 * frame[..., 1]) + 0.25 * frame[..., 2]
                ok = (plane == 1) & (Y >= LO) & (Y <= HI)
                valid.append(ok)
                q.append(torch.where(ok, Y * 65536.0, torch.zeros_like(Y)).to(torch.int64))
            for i in range(6):
                for j in range(6):
                    both = valid[i] & valid[j]
                    stats[i, j, 0] = both.sum()
                    stats[i, j, 1] = (q[i] * both).sum()
            return stats
    elif a.row == "plain":
        def run():
            lrp.compose_cameras(cams, out_image, a.n, a.interp, rots, mode)
            return out
    else:
        def run():
            lrp.compose_cameras(cams, out_image, a.n, a.interp, rots, mode, gains=gains)
            return out

    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        result = run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    if a.row in ("stat", "hand"):
        table = result.cpu().numpy()
        check = f"table checksum {int(np.bitwise_xor.reduce((table.reshape(-1) * np.arange(1, 129)).astype(np.uint64))):016x}  N_00 {table[0, 0, 0]}  N_01 {table[0, 1, 0]}"
    else:
        check = f"checksum {lrp.checksums([out])[0]:016x}"
    what = {"stat": "overlap, one launch", "hand": "overlap by hand", "plain": "compose_cameras", "gain": "compose_cameras gains"}[a.row]
    shape = "" if a.row in ("stat", "hand") else f"{('nn', 'bl', 'bc')[a.interp]} {a.mode} n {a.n} "
    print(f"row {a.row:5s} {what:22s} {shape}{ow}x{oh} avg {np.mean(times):9.1f} us  median {np.median(times):9.1f} us  min {np.min(times):9.1f} us  {check}",
          flush=True)


if __name__ == "__main__":
    main()
