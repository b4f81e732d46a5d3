#!/usr/bin/env python3
"""Times compose into a calibrated target camera against its ideal-target twins: the sources of rows a
and b of tools/camera_bench.py — RGBA frames, bicubic, FEATHER, num_samples n = 1 or 2 — into a 4096 x 2048 target,

  a   six 2048^2 BROWN cameras (a cube's faces with the barrel distortion of a wide lens);
  b   two 3008^2 FISHEYE cameras of 200 degrees, back to back;

  brown     the target is a BROWN camera (fx = fy = 1720, the coefficients of the sources) through lrp_camera_view_device;
  fisheye   the target is a FISHEYE camera (fx = fy = 4096 / 200 degrees, the coefficients of row b's sources) through
            lrp_camera_view_device;
  --twin    the same sources through lrp_compose_cameras_device into the ideal lens of the same size and horizontal field of
            view — rectilinear for brown, equidistant for fisheye; the field is the one lrp_camera_unproject reports for the
            middle of the target's right edge.  The twin is the kernel the camera-view kernel was derived from: the two differ
            in the target ray alone (and, through the distortion, slightly in which texels are gathered off axis).

One row per process; alternate row and twin in rounds.

usage: camera_view_bench.py a|b brown|fisheye 1|2 [--twin] [--interp I] [--mode first|mean|feather] [--reps R] [--warmup W]
Prints one line: average, median and minimum us per launch (events around every launch), output samples per second, the share
of covered pixels, the mean number of sources that cover a pixel (every one of them is sampled under MEAN and FEATHER) and the
checksum of the result."""
import argparse
import importlib
import math
import os
import sys

import numpy as np

BROWN_K = (-0.12, 0.03, 0.0005, -0.0003, -0.004)  # k1 k2 p1 p2 k3: an ordinary wide lens
FISHEYE_K = (-0.02, 0.003, -0.0005, 0.00005)       # k1 .. k4
FISHEYE_FOV = math.radians(200.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=["a", "b"])
    ap.add_argument("target", choices=["brown", "fisheye"])
    ap.add_argument("n", type=int, choices=[1, 2])
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--interp", type=int, default=2, choices=[0, 1, 2])
    ap.add_argument("--mode", default="feather", choices=["first", "mean", "feather"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    lrp = importlib.import_module("image-lens-reproject_amd")
    C, ow, oh = 4, 4096, 2048
    d2r = np.float32(np.pi / 180.0)
    six = a.row == "a"
    f = 2048 if six else 3008
    angles = [(0, 0), (90, 0), (180, 0), (270, 0), (0, 90), (0, -90)] if six else [(0, 0), (180, 0)]  # pan, pitch
    rots = [lrp.rotation_matrix(float(np.float32(p) * d2r), float(np.float32(t) * d2r), 0.0) for p, t in angles]
    srcs = []
    for i in range(len(angles)):
        t = torch.empty((f, f, C), dtype=torch.float32, device="cuda")
        lrp.synth_fill(t, f, f, C, 0xCA00 + i)
        srcs.append(t)
    out = torch.empty((oh, ow, C), dtype=torch.float32, device="cuda")
    mode = {"first": 0, "mean": 1, "feather": 2}[a.mode]
    centre = f / 2 - 0.5
    if six:
        cams = [lrp.Camera.brown(f, f, t, f / 2.0, f / 2.0, centre, centre, BROWN_K) for t in srcs]
    else:
        cams = [lrp.Camera.fisheye(f, f, t, f / FISHEYE_FOV, f / FISHEYE_FOV, centre, centre, FISHEYE_K, limit=FISHEYE_FOV / 2) for t in srcs]

    tcx, tcy = ow / 2 - 0.5, oh / 2 - 0.5
    if a.target == "brown":
        target = lrp.Camera.brown(ow, oh, None, 1720.0, 1720.0, tcx, tcy, BROWN_K)
    else:
        target = lrp.Camera.fisheye(ow, oh, None, ow / FISHEYE_FOV, ow / FISHEYE_FOV, tcx, tcy, FISHEYE_K)  # (limit: lrp_camera_limit)
    edge, has = lrp.camera_unproject(target, np.array([[ow - 0.5, tcy]], dtype=np.float32))  # the middle of the right edge
    assert has[0]
    half = math.atan2(float(edge[0, 0]), -float(edge[0, 2]))  # half the horizontal field of view
    if a.target == "brown":
        twin = lrp.LensInfo.rectilinear(18.0 / math.tan(half), 36.0, ow, oh)  # tan(half) = 18 / focal on a 36 mm sensor
    else:
        twin = lrp.LensInfo.equidistant(2.0 * half)
    out_image = lrp.Image(twin, ow, oh, C, out)

    if a.twin:
        def run():
            return lrp.compose_cameras(cams, out_image, a.n, a.interp, rots, mode, count=plane, coverage=plane)
    else:
        def run():
            return lrp.camera_view(cams, target, out, a.n, a.interp, rots, mode, count=plane, coverage=plane)

    plane = True
    k, m = run()  # once with the planes, for the share of covered pixels and the sources per pixel
    torch.cuda.synchronize()
    covered, sources = float((m > 0).float().mean()), float(k.float().mean())
    plane = None
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
    what = f"{'twin' if a.twin else 'view'} {'brown6x2048' if six else 'fisheye2x3008'} -> {a.target}"
    print(f"row {a.row} {what:36s} {('nn', 'bl', 'bc')[a.interp]} {a.mode:7s} n {a.n} {ow}x{oh} half fov {math.degrees(half):6.2f} deg  "
          f"avg {np.mean(times):9.1f} us  median {np.median(times):9.1f} us  min {np.min(times):9.1f} us  "
          f"{ow * oh * a.n * a.n / np.mean(times) / 1e3:7.2f} Gsamples/s  covered {covered:.4f}  sources {sources:.3f}  "
          f"checksum {lrp.checksums([out])[0]:016x}", flush=True)


if __name__ == "__main__":
    main()
