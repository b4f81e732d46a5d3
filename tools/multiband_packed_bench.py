#!/usr/bin/env python3
"""Times multi-band blending on packed frames on the scene of tools/multiband_bench.py: six 2048^2 BROWN
cameras (a cube's faces with the barrel distortion of a wide lens) into an equirectangular output of 4096 x 2048 or 1024 x 512,
four samples per pixel, RGBA8 frames into an RGBA8 panorama or binary16 frames into a binary16 one —

  packed  lrp_compose_cameras_multiband_packed_device, B = --bands (5), --interp (bicubic), a scratch buffer allocated once;
  chain   the chain it is defined by, on the same commit: six lrp_decode_pixels_device into float32 frames allocated once, then
          lrp_compose_cameras_multiband_device into a float32 panorama allocated once, then lrp_encode_pixels_device.

One row per process; alternate them in rounds.

usage: multiband_packed_bench.py packed|chain [--format rgba8|half] [--size 4096x2048|1024x512] [--bands B] [--interp I]
                                 [--root DIR] [--reps R] [--warmup W]
Prints one line: minimum, median and maximum us per repetition (events around every repetition), the bytes of frames, float32
temporaries, scratch and output the route holds, and a checksum of the output's bytes (the two rows print the same one)."""
import argparse
import importlib
import os
import sys
import zlib

import numpy as np

BROWN_K = (-0.12, 0.03, 0.0005, -0.0003, -0.004)  # tools/camera_bench.py row a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("row", choices=["packed", "chain"])
    ap.add_argument("--format", default="rgba8", choices=["rgba8", "half"])
    ap.add_argument("--size", default="4096x2048", choices=["4096x2048", "1024x512"])
    ap.add_argument("--bands", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--interp", type=int, default=2, choices=[0, 1, 2])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import torch

    lrp = importlib.import_module("image-lens-reproject_amd")
    C, f, B = 4, 2048, a.bands
    ow, oh = (int(v) for v in a.size.split("x"))
    fmt, dtype = (lrp.PixelFormat.U8_GAMMA, torch.uint8) if a.format == "rgba8" else (lrp.PixelFormat.F16, torch.int16)
    d2r = np.float32(np.pi / 180.0)
    angles = [(0, 0), (90, 0), (180, 0), (270, 0), (0, 90), (0, -90)]  # pan, pitch
    rots = [lrp.rotation_matrix(float(np.float32(p) * d2r), float(np.float32(t) * d2r), 0.0) for p, t in angles]
    frames = []
    t = torch.empty((f, f, C), dtype=torch.float32, device="cuda")
    for i in range(6):  # the frames of tools/multiband_bench.py, in the format
        lrp.synth_fill(t, f, f, C, 0xCA00 + i)
        frames.append(torch.empty((f, f, C), dtype=dtype, device="cuda"))
        lrp.encode_pixels(t, frames[-1], fmt)
    torch.cuda.synchronize()
    del t
    centre = f / 2 - 0.5
    pano = lrp.LensInfo.equirectangular()
    out = torch.empty((oh, ow, C), dtype=dtype, device="cuda")
    scratch = torch.empty(lrp.multiband_scratch_bytes(ow, oh, C, B), dtype=torch.uint8, device="cuda")
    held = dict(frames=sum(x.numel() * x.element_size() for x in frames), scratch=scratch.numel(), output=out.numel() * out.element_size())

    if a.row == "packed":
        cams = [lrp.Camera.brown(f, f, None, f / 2.0, f / 2.0, centre, centre, BROWN_K) for _ in frames]
        out_image = lrp.Image(pano, ow, oh, C, None)
        held["float32 temporaries"] = 0

        def run():
            lrp.compose_cameras_multiband_packed(cams, fmt, frames, out_image, fmt, out, 0, a.interp, rots, B, scratch=scratch)
    else:
        tmps = [torch.empty((f, f, C), dtype=torch.float32, device="cuda") for _ in frames]
        tmp_out = torch.empty((oh, ow, C), dtype=torch.float32, device="cuda")
        cams = [lrp.Camera.brown(f, f, x, f / 2.0, f / 2.0, centre, centre, BROWN_K) for x in tmps]
        out_image = lrp.Image(pano, ow, oh, C, tmp_out)
        held["float32 temporaries"] = sum(x.numel() * 4 for x in tmps) + tmp_out.numel() * 4

        def run():
            for src, tmp in zip(frames, tmps):
                lrp.decode_pixels(src, fmt, tmp)
            lrp.compose_cameras_multiband(cams, out_image, a.interp, rots, B, scratch=scratch)
            lrp.encode_pixels(tmp_out, out, fmt)

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
    mb = lambda n: f"{n / 1e6:.1f}"  # noqa: E731
    print(f"row {a.row:6s} {a.format:5s} B {B} {('nn', 'bl', 'bc')[a.interp]} {ow}x{oh} min {np.min(times):9.1f} us  median {np.median(times):9.1f} us  "
          f"max {np.max(times):9.1f} us  MB held: frames {mb(held['frames'])} float32 temporaries {mb(held['float32 temporaries'])} scratch "
          f"{mb(held['scratch'])} output {mb(held['output'])}  crc32 {zlib.crc32(out.cpu().numpy().tobytes()):08x}", flush=True)


if __name__ == "__main__":
    main()
