#!/usr/bin/env python3
"""Times the packed camera calls against the chains they are defined by, on the rig of
tools/camera_gain_bench.py: six 2048^2 BROWN cameras (a cube's faces with the barrel distortion of a wide lens) whose frames
are RGBA8 or RGBA half, into an equirectangular RGBA output of the same format, 4096 x 2048 or 1024 x 512 —

  fused   one launch: lrp_compose_cameras_packed_device (with gains 0.8 .. 1.3), or lrp_camera_overlap_packed_device for --what stat;
  chain   what it is defined by, on the same frames: six lrp_decode_pixels_device, lrp_compose_cameras_gain_device (or
          lrp_camera_overlap_device) and one lrp_encode_pixels_device, with float32 staging frames allocated once.

usage: camera_packed_bench.py row chain|fused [--what bc_feather|bl_first|stat] [--n 1|2] [--fmt u8|f16] [--size WxH] [--reps R] [--warmup W]
       camera_packed_bench.py all [--rounds 3] [--limit SECONDS] [--out FILE]
`row` measures one row in this process and prints one line: min, median and max us per repetition (events around every
repetition), the bytes of float32 staging the row allocates, and a checksum of the output bytes or of the table, which chain
and fused must share.  `all` runs every row of the section in rounds that alternate chain and fused, each row in a fresh
process under its own time limit; it stops at the first row that fails or runs out of time, and at a checksum that differs."""
import argparse
import importlib
import os
import subprocess
import sys

import numpy as np

BROWN_K = (-0.12, 0.03, 0.0005, -0.0003, -0.004)  # tools/camera_bench.py row a
LO, HI = 0.02, 0.98
U8, F16 = 2, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def row(a):
    sys.path.insert(0, ROOT)
    import torch

    lrp = importlib.import_module("image-lens-reproject_amd")
    C, f = 4, 2048
    ow, oh = (int(v) for v in a.size.split("x"))
    fmt = U8 if a.fmt == "u8" else F16
    d2r = np.float32(np.pi / 180.0)
    angles = [(0, 0), (90, 0), (180, 0), (270, 0), (0, 90), (0, -90)]  # pan, pitch
    rots = [lrp.rotation_matrix(float(np.float32(p) * d2r), float(np.float32(t) * d2r), 0.0) for p, t in angles]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0xCA00)
    if fmt == U8:
        frames = [torch.randint(0, 256, (f, f, C), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(6)]
        out = torch.empty((oh, ow, C), dtype=torch.uint8, device="cuda")
    else:
        frames = [torch.rand((f, f, C), dtype=torch.float32, device="cuda", generator=gen).to(torch.float16).view(torch.int16) for _ in range(6)]
        out = torch.empty((oh, ow, C), dtype=torch.int16, device="cuda")
    centre = f / 2 - 0.5
    pano = lrp.LensInfo.equirectangular()
    gains = np.linspace(0.8, 1.3, 6).astype(np.float32)
    interp, mode = {"bc_feather": (2, 2), "bl_first": (1, 0), "stat": (1, 0)}[a.what]
    stats = torch.empty((8, 8, 2), dtype=torch.int64, device="cuda")
    staging = 0
    if a.row == "fused":
        cams = [lrp.Camera.brown(f, f, None, f / 2.0, f / 2.0, centre, centre, BROWN_K) for _ in frames]
        out_image = lrp.Image(pano, ow, oh, C, None)
        if a.what == "stat":
            def run():
                lrp.camera_overlap_packed(cams, fmt, frames, out_image, rots, LO, HI, stats=stats)
        else:
            def run():
                lrp.compose_cameras_packed(cams, fmt, frames, out_image, fmt, out, 0, a.n, interp, rots, mode, gains=gains)
    else:
        tmps = [torch.empty((f, f, C), dtype=torch.float32, device="cuda") for _ in frames]
        cams = [lrp.Camera.brown(f, f, t, f / 2.0, f / 2.0, centre, centre, BROWN_K) for t in tmps]
        staging = sum(t.numel() * 4 for t in tmps)
        if a.what == "stat":
            out_image = lrp.Image(pano, ow, oh, C, None)

            def run():
                for d, t in zip(frames, tmps):
                    lrp.decode_pixels(d, fmt, t)
                lrp.camera_overlap(cams, out_image, rots, LO, HI, stats=stats)
        else:
            tmp_out = torch.empty((oh, ow, C), dtype=torch.float32, device="cuda")
            staging += tmp_out.numel() * 4
            out_image = lrp.Image(pano, ow, oh, C, tmp_out)

            def run():
                for d, t in zip(frames, tmps):
                    lrp.decode_pixels(d, fmt, t)
                lrp.compose_cameras(cams, out_image, a.n, interp, rots, mode, gains=gains)
                lrp.encode_pixels(tmp_out, out, fmt, fill=0)

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
    if a.what == "stat":
        table = stats.cpu().numpy().reshape(-1).astype(np.uint64)
        check = int(np.bitwise_xor.reduce(table * np.arange(1, 129, dtype=np.uint64)))
    else:
        flat = out.reshape(-1).to(torch.int64) & 0xFFFF
        check = int((flat * (torch.arange(flat.numel(), device="cuda") % 251 + 1)).sum().item())
    shape = "stat" if a.what == "stat" else f"{a.what} n {a.n}"
    print(f"row {a.row:5s} {a.fmt:3s} {shape:16s} {ow}x{oh} min {np.min(times):9.1f} us  median {np.median(times):9.1f} us  max {np.max(times):9.1f} us  "
          f"staging {staging / 2**20:6.0f} MiB  checksum {check:016x}", flush=True)


def everything(a):
    """Every row of DESIGN.md section 21, a fresh process per row, each under its own time limit."""
    configs = [(what, n) for what, n in (("bc_feather", 1), ("bc_feather", 2), ("bl_first", 1), ("stat", 1))]
    sink = open(a.out, "a") if a.out else None
    for fmt in ("u8", "f16"):
        for size in ("4096x2048", "1024x512"):
            for what, n in configs:
                for r in range(a.rounds):
                    sums = {}
                    for which in ("chain", "fused"):
                        cmd = [sys.executable, os.path.abspath(__file__), "row", which, "--what", what, "--n", str(n), "--fmt", fmt, "--size", size]
                        try:
                            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
                        except subprocess.TimeoutExpired:
                            print(f"TIME LIMIT ({a.limit} s): {' '.join(cmd[2:])}; nothing further is started", flush=True)
                            return 1
                        line = p.stdout.strip()
                        if p.returncode != 0 or "checksum" not in line:
                            print(f"FAILED ({p.returncode}): {' '.join(cmd[2:])}\n{p.stdout}{p.stderr}\nnothing further is started", flush=True)
                            return 1
                        line = f"round {r} {line}"
                        print(line, flush=True)
                        if sink:
                            sink.write(line + "\n")
                            sink.flush()
                        sums[which] = line.rsplit("checksum", 1)[1].strip()
                    if sums["chain"] != sums["fused"]:
                        print("the checksums of chain and fused differ; nothing further is started", flush=True)
                        return 1
    return 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("row")
    r.add_argument("row", choices=["chain", "fused"])
    r.add_argument("--what", default="bc_feather", choices=["bc_feather", "bl_first", "stat"])
    r.add_argument("--n", type=int, default=1, choices=[1, 2])
    r.add_argument("--fmt", default="u8", choices=["u8", "f16"])
    r.add_argument("--size", default="4096x2048", choices=["4096x2048", "1024x512"])
    r.add_argument("--reps", type=int, default=30)
    r.add_argument("--warmup", type=int, default=10)
    e = sub.add_parser("all")
    e.add_argument("--rounds", type=int, default=3)
    e.add_argument("--limit", type=int, default=120)
    e.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cmd == "row":
        row(a)
        return 0
    return everything(a)


if __name__ == "__main__":
    sys.exit(main())
