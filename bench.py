#!/usr/bin/env python3
"""bench.py — Mpix/s of the lens-reprojection hot path on MI355X.

Contract (see the task statement): `python bench.py --gpus N --steps K --warmup W`;
for N > 1 it is launched by torch.distributed.run, one rank per GPU (started without
torchrun it starts torchrun itself, as a child, before anything touches the GPU).
Prints ONE JSON line on rank 0.

A step = one pass of the hot path over one batch of `--batch` (default 256, north_star's
"256-image batch") synthetic 4096x4096 RGBA float frames that are already resident in
HBM (generated on the device by the counter-based generator; image i has seed
0x5EED0000 + i on whichever rank renders it).  The batch is one sorted list of
independent images sharded in contiguous static blocks, block r -> rank r, exactly as
the reference hands files to its pool threads (src/main.cpp:538-544, 624-655;
image-lens-reproject_amd/sharding.py): STRONG scaling, total work fixed, no
collective on the data path.  `--scaling weak` gives every rank its own `--batch`
frames instead.  The frames of a step share one geometry (a directory of frames from
one camera, the reference's --input-dir path), so a rank renders its block with one
kernel launch per 16 frames (lrp_reproject_batch_device); `--per-frame-launches`
issues one launch per frame instead, round-robin over `--streams` HIP streams.

A plain run sets up, warms up, times the steps and prints the line; next to the headline value
(and ms_per_step, the wall time of one timed step) it reports
  roofline            dominant kernel of the headline workload, from the HIP events around the
                      launches of the timed region (frac = read + write algorithmic bytes / time / 8 TB/s,
                      frac_read_only = source bytes only)
`--dump-outputs DIR` writes a seeded sample of what the last timed step rendered (dump_outputs).
`--full` measures and checks the rest, all in this process:
  roofline            + single_launch_us = one frame per launch (and two-stream / uncached variants)
  secondary           the same figures for the other workloads of DEFAULT_SECONDARY
  outputs_digest      sha256 over the per-image 64-bit checksums of the rendered batch, in
                      image order: equal for any N (tests/test_bench_multi_rank.py), and
                      compared with the oracle's committed checksums (exit status 3 if they differ)
  staged              host-buffer (PCIe-inclusive) rates, tools/staged_bench
  cpu_baseline        the oracle on this host's cores, one image per thread
"""
import argparse
import hashlib
import importlib
import json
import math
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FRAMES_PER_LAUNCH = 16  # lrp::kMaxBatch

WORKLOADS = {
    # BASELINE.json configs[1] (the config the metric is quoted on).  The reference
    # rejects FISHEYE_EQUISOLID (src/reproject.cpp:395-397), so the fisheye is the
    # equidistant one with fov = pi, as SURVEY.md §8d prescribes for parity.
    "fisheye_to_rect_bicubic": dict(in_lens="eqd", out_lens="rect", interp=2, rot=None, channels=4, size=4096),
    # north_star's roofline target case.
    "equirect_to_rect_bicubic": dict(in_lens="eqr", out_lens="rect", interp=2, rot=(0.0, 0.0, 0.0), channels=4,
                                     size=4096),
    # what every real --rotation runs (the CLI always passes a matrix, src/main.cpp:312-325)
    "equirect_to_rect_bicubic_rot": dict(in_lens="eqr", out_lens="rect", interp=2, rot=(30.0, -15.0, 5.0), channels=4,
                                         size=4096),
    # BASELINE.json configs[2] shape.
    "equirect_to_fisheye_bilinear": dict(in_lens="eqr", out_lens="eqd", interp=1, rot=(30.0, -15.0, 5.0), channels=4,
                                         size=4096),
    # SURVEY.md §8d scaling workload: the configs[2] shape with bicubic.
    "equirect_to_fisheye_bicubic_rot": dict(in_lens="eqr", out_lens="eqd", interp=2, rot=(30.0, -15.0, 5.0), channels=4,
                                            size=4096),
    # BASELINE.json configs[0] shape at 4K (plumbing case, nearest).
    "equirect_to_rect_nearest": dict(in_lens="eqr", out_lens="rect", interp=0, rot=(0.0, 0.0, 0.0), channels=4,
                                     size=4096),
    # BASELINE.json configs[3]: RGBAZ, rectilinear -> equirect(full), bicubic, exposure 2^1, Reinhard 4 fused into the store.
    "rect_to_equirect_bicubic_rgbaz_post": dict(in_lens="rect", out_lens="eqr", interp=2, rot=(0.0, 0.0, 0.0), channels=5,
                                                depth=4, post=(2.0, 4.0), size=4096),
    # the same mapping, RGBA, no tonemap
    "rect_to_equirect_bicubic": dict(in_lens="rect", out_lens="eqr", interp=2, rot=(0.0, 0.0, 0.0), channels=4,
                                     size=4096),
    # the reference's --samples 2 on the down-scale its README asks it for (src/reproject.cpp:294-298): 4096^2 -> 2048^2, four
    # sub-samples per pixel through the window kernel's SS instantiations (a lane per sub-sample; an entry of sub-samples in the
    # geometry cache)
    "fisheye_to_rect_bicubic_half_ns2": dict(in_lens="eqd", out_lens="rect", interp=2, rot=None, channels=4, size=4096, out_size=2048, ns=2),
    # ... and the other two settings the reference's help text prescribes (src/main.cpp:192-196): --scale 0.33334 --samples 3 (4096 ->
    # int(4096 * 0.33334) = 1365, src/main.cpp:581-587) and --scale 0.25 --samples 4
    "fisheye_to_rect_bicubic_third_ns3": dict(in_lens="eqd", out_lens="rect", interp=2, rot=None, channels=4, size=4096, out_size=1365, ns=3),
    "fisheye_to_rect_bicubic_quarter_ns4": dict(in_lens="eqd", out_lens="rect", interp=2, rot=None, channels=4, size=4096, out_size=1024, ns=4),
    # BASELINE.json configs[4]: one 8192^2 RGB panorama -> six 2048^2 rectilinear faces, bicubic; a "frame" is a cubemap
    "cubemap_8k_rgb": dict(in_lens="eqr", out_lens="rect", interp=2, channels=3, size=8192, out_size=2048,
                           faces=[(0.0, 0.0, 0.0), (90.0, 0.0, 0.0), (180.0, 0.0, 0.0), (270.0, 0.0, 0.0), (0.0, 90.0, 0.0),
                                  (0.0, -90.0, 0.0)], rot=None),
}
DEFAULT_SECONDARY = ("equirect_to_rect_bicubic,equirect_to_rect_bicubic_rot,equirect_to_fisheye_bilinear,"
                     "equirect_to_fisheye_bicubic_rot,rect_to_equirect_bicubic_rgbaz_post,cubemap_8k_rgb,fisheye_to_rect_bicubic_half_ns2,"
                     "fisheye_to_rect_bicubic_third_ns3,fisheye_to_rect_bicubic_quarter_ns4")
INTERP_NAMES = {0: "nearest", 1: "bilinear", 2: "bicubic"}
KERNEL_NAMES = {0: "reproject_tile_kernel (nearest)", 1: "reproject_tile_kernel (bilinear)",
                2: "reproject_bicubic_win_kernel (LDS window)"}
TRAFFIC_FILE = os.path.join("profiles", "traffic_r06.json")


def kernel_source_sha():
    """Hash of everything that decides which kernel a workload runs and what it does: every source, header and the build
    script (per-unit code generation options) of csrc/.  The PMC traffic file is only valid for the sources it was measured on."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "image-lens-reproject_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".h", ".hip", ".cpp", ".sh")):
            with open(os.path.join(csrc, name), "rb") as f:
                h.update(name.encode())
                h.update(f.read())
    return h.hexdigest()[:16]


def measured_traffic(workload):
    """(per 16-frame launch, per single-frame launch) HBM bytes of the dominant kernel from the committed rocprofv3 PMC
    summary (profiles/traffic_r05.json; tools/collect_traffic.sh on an MI355X: both launch shapes are profiled).  The
    file is stamped with the hash of the kernel sources it was measured on; a stale file yields (None, None)."""
    try:
        with open(os.path.join(ROOT, TRAFFIC_FILE)) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None, None
    if d.get("_kernel_source_sha") != kernel_source_sha():
        return None, None
    return d.get(workload + "@batch16"), d.get(workload)


def make_lens(pkg, kind, w, h):
    if kind == "rect":
        return pkg.LensInfo.rectilinear(18.0, 36.0, w, h)
    if kind == "eqd":
        return pkg.LensInfo.equidistant(3.14159265)
    return pkg.LensInfo.equirectangular()


def make_rot(pkg, deg):
    if deg is None:
        return None
    r = [d * math.pi / 180.0 for d in deg]
    return pkg.rotation_matrix(*r)


def usable_cpus():
    """CPUs this process may actually use: affinity mask, capped by the cgroup v2 CPU quota
    (a GPU box hands a 1-GPU job a 16-CPU share of a 256-thread host)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(pkg, wl, seconds_target):
    """The oracle (kind "port": our C restatement of the reference loop, built with the
    reference's flags) timed on this host's cores the way the reference schedules work
    (SURVEY §8d): ONE IMAGE PER THREAD, -j = usable cores (src/main.cpp:538-544), each
    thread with its own source and destination frame; plus the single-thread figure.
    Bounded sample: every thread renders the first `rows` rows of its own frame."""
    import ctypes

    import numpy as np
    import oracle_binding as oracle

    cores = usable_cpus()
    size, c = wl["size"], wl["channels"]
    lin, lout = make_lens(pkg, wl["in_lens"], size, size), make_lens(pkg, wl["out_lens"], size, size)
    rot = make_rot(pkg, wl["rot"])
    L = oracle.lib()
    keep, rp = oracle._rot(rot)

    def run(n_threads, rows):
        """n_threads images in flight, one per thread, each thread rendering `rows` output rows in
        total (whole frames of its own image, then a partial one); returns the wall seconds of the
        slowest thread (all start together)."""
        start = threading.Barrier(n_threads + 1)
        done = [0.0] * n_threads

        def work(t):
            src = oracle.synth_frame(size, size, c, 0x5EED0000 + t)  # this thread's own image
            out = np.empty((size, size, c), dtype=np.float32)
            cin, cout = oracle._image(lin, size, size, c, src), oracle._image(lout, size, size, c, out)
            start.wait()
            left = rows
            while left > 0:
                n = min(left, size)
                L.lrpo_reproject_rows(ctypes.byref(cin), ctypes.byref(cout), wl.get("ns", 1), wl["interp"], rp, 0, n)
                left -= n
            done[t] = time.perf_counter()

        threads = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
        for th in threads:
            th.start()
        start.wait()
        t0 = time.perf_counter()
        for th in threads:
            th.join()
        return max(done) - t0

    probe_rows = max(16, size // 32)
    dt_probe = run(1, probe_rows)  # calibration: rows per second of one thread
    # ~seconds_target of CPU work in all: a third single-threaded, two thirds with every core busy
    rows_one = int(max(probe_rows, probe_rows * (seconds_target / 3.0) / max(dt_probe, 1e-4)))
    rows = int(max(probe_rows, probe_rows * (seconds_target * 2.0 / 3.0) / max(dt_probe, 1e-4)))
    dt_one = run(1, rows_one)
    dt_all = run(cores, rows)
    return {
        "value": cores * rows * size / dt_all / 1e6,
        "unit": "Mpix/s",
        "cores": cores,
        "kind": "port",
        "single_thread_value": rows_one * size / dt_one / 1e6,
        "cpu_model": cpu_model(),
        "sample": f"{cores} threads (usable CPUs) x {rows / size:.2f} frames of {size}x{size}x{c}, one image per thread as the "
                  f"reference's -j pool ({dt_all:.1f} s); 1 thread: {rows_one / size:.2f} frames ({dt_one:.1f} s)",
        "sample_detail": f"one image per thread like the reference's -j pool (src/main.cpp:538-544): {cores} threads = usable CPUs "
                         f"(affinity {len(os.sched_getaffinity(0))}, cgroup quota honoured), each rendering {rows / size:.2f} frames "
                         f"of its own {size}x{size}x{c} image ({dt_all:.1f} s wall); single thread: {rows_one / size:.2f} frames of one "
                         f"image ({dt_one:.1f} s)",
    }


def staged_rates():
    """Host-buffer (PCIe-inclusive) rates of the batch pipeline — what a caller with frames in host memory sees, never
    `value` —: tools/staged_bench on 4096^2 RGBA frames, best stream count per format.  A separate ~3 s process, after
    the timed region.  None if the tool is not built."""
    import re

    exe = os.path.join(ROOT, "tools", "staged_bench")
    if not os.path.exists(exe):
        return None
    try:
        text = subprocess.run([exe, "6"], capture_output=True, text=True, timeout=120).stdout
    except (OSError, subprocess.TimeoutExpired):
        return None
    best = {}
    for line in text.splitlines():
        m = re.match(r"(.*?)\s+streams=(\d+): (\d+) Mpix/s staged", line)
        if m:
            key = {"pinned=0": "f32_pageable", "pinned=1": "f32_pinned"}.get(m.group(1).strip(), None)
            if key is None:
                key = "binary16_pinned" if "binary16" in m.group(1) else ("rgba8_pinned" if "RGBA8" in m.group(1) else m.group(1).strip())
            best[key] = max(best.get(key, 0.0), float(m.group(3)))
    if not best:
        return None
    return {"unit": "Mpix/s", "workload": "fisheye_to_rect_bicubic 4096^2 RGBA, host buffers in and out (lrp_context_submit*)", **best,
            "note": "PCIe-inclusive: upload + kernel + download pipelined over three streams; bound by the PCIe link, not by the kernel"}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=0,
                    help="timed steps (default: 20, more when a rank's shard is small so that the timed region is >= ~0.5 s)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256,
                    help="images per step: the whole job's batch (strong scaling, sharded over the ranks in static "
                         "blocks) or every rank's own batch (--scaling weak)")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"])
    ap.add_argument("--distinct", type=int, default=0,
                    help="distinct resident source / destination frame pairs per GPU (0 = the rank's whole shard if it "
                         "fits in 70 %% of the free HBM, else as many as fit, at least 16)")
    ap.add_argument("--per-frame-launches", action="store_true",
                    help="one kernel launch per frame (lrp_reproject_device) instead of one per 16 frames "
                         "(lrp_reproject_batch_device: all frames of a step share one geometry)")
    ap.add_argument("--streams", type=int, default=1,
                    help="HIP streams the frames of a step round-robin over (--per-frame-launches only)")
    ap.add_argument("--workload", default="fisheye_to_rect_bicubic", choices=sorted(WORKLOADS))
    ap.add_argument("--secondary", default=None,
                    help="comma-separated workloads measured (kernel timing only) in the same process; '' = none "
                         "(default: those of DEFAULT_SECONDARY with --full at N = 1, none otherwise)")
    ap.add_argument("--size", type=int, default=0, help="override the frame size (tests; 0 = the workload's 4096)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend of the barrier / max-time reduction for --gpus > 1 (nccl = RCCL; "
                         "gloo lets two ranks share one GPU in a smoke test of the multi-rank path)")
    ap.add_argument("--checksums-file", default="", help="rank 0 writes the per-image checksum list (JSON) here")
    ap.add_argument("--settle-seconds", type=float, default=2.0,
                    help="untimed launches of the workload before the warm-up steps: the chip takes its sustained "
                         "(power-limited) clock only after a while under load, and a first launch after idle is 10-25 %% slower")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-staged", action="store_true", help="skip the host-buffer (PCIe-inclusive) leg (tools/staged_bench)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--detail-file", default=None,
                    help="rank 0 writes the full result here (notes, traffic detail, two-stream / uncached single launches, per-rank "
                         "times, staged rates); stdout carries the compact line only.  '' = do not write (default: "
                         "bench_detail.json with --full, none otherwise)")
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beyond the headline figure as well: the single-launch / two-stream / "
                         "uncached legs, the secondary workloads, the host-buffer leg, the CPU baseline, the per-image checksums "
                         "against the committed oracle fixture and the detail file (default: set up, warm up, time the steps, "
                         "print the line)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, rank 0 writes what the last step rendered as DIR/<name>.npy: a fixed, seeded "
                         "sample of pixels of every image of the batch and a full-resolution crop of image 0 (float32), and the "
                         "sampled positions (float64); < 64 MB in all")
    ap.add_argument("--force-dist", action="store_true",
                    help="--gpus 1 through the N > 1 code path: started under torch.distributed.run with one rank, process group "
                         "initialised (nccl = RCCL), barriers and the device-side MAX reduction run on a world-size-1 communicator — "
                         "the one RCCL launch a one-GPU box admits (tests/test_bench_multi_rank.py)")
    ap.add_argument("--full-legs", action="store_true",
                    help="N > 1: measure the single-launch / two-stream / uncached legs and the secondary workloads on rank 0 as at "
                         "N = 1 (default for N > 1: the timed region only, so that the other ranks are released at once)")
    return ap.parse_args()


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` without a launcher: start torch.distributed.run as a CHILD (this
    process has not touched the GPU) and exit with its code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def time_launches(torch, stream, fn, reps):
    """Average / min duration (ms) of `fn(i)` (one kernel launch each) by events on `stream`."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i in range(reps):
        ev[i][0].record(stream)
        fn(i)
        ev[i][1].record(stream)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return sum(ms) / len(ms), ms[0]


def resident_frames(torch, pkg, wl, size, n, dev, first_seed=0x5EED0000):
    """n distinct synthetic source / destination pairs of one workload, resident in HBM."""
    c, out_size = wl["channels"], wl.get("out_size") and (wl["out_size"] * size // wl["size"]) or size
    faces = len(wl.get("faces") or [None])
    srcs, dsts = [], []
    for k in range(n):
        s = torch.empty((size, size, c), dtype=torch.float32, device=dev)
        pkg.synth_fill(s, size, size, c, first_seed + k, wl.get("depth", -1))
        srcs.append(s)
        dsts.append([torch.empty((out_size, out_size, c), dtype=torch.float32, device=dev) for _ in range(faces)])
    return srcs, dsts


def kernel_figures(torch, pkg, wl, size, srcs, dsts, stream, name, timed_region_ms=None, single_legs=True):
    """Roofline figures of one workload's dominant kernel on resident frames: 16-frame launches and
    single-frame launches, both with HIP events on the launch stream, cycling over the resident frames.
    `dsts[k]` is the list of outputs of source k (one; six for the cubemap, where a "frame" is one
    cubemap = six launches over one resident source and frames_per_launch is 1)."""
    c = wl["channels"]
    out_size = dsts[0][0].shape[0]
    lin, lout = make_lens(pkg, wl["in_lens"], size, size), make_lens(pkg, wl["out_lens"], out_size, out_size)
    post = wl.get("post")
    ns = wl.get("ns", 1)
    faces = wl.get("faces")
    n_res = len(srcs)
    im_in = [pkg.Image(lin, size, size, c, s) for s in srcs]
    im_out = [[pkg.Image(lout, out_size, out_size, c, d) for d in ds] for ds in dsts]
    if faces:
        import numpy as np

        rots = np.stack([make_rot(pkg, f) for f in faces])
        nb = 1

        def batched(i):
            pkg.reproject_multi(im_in[i % n_res], im_out[i % n_res], ns, wl["interp"], rots, post=post, stream=stream)

        single = batched
    else:
        rot = make_rot(pkg, wl["rot"])
        nb = min(FRAMES_PER_LAUNCH, n_res)

        def batched(i):
            ids = [(i * nb + k) % n_res for k in range(nb)]
            pkg.reproject_batch([im_in[j] for j in ids], [im_out[j][0] for j in ids], ns, wl["interp"], rot, post=post, stream=stream)

        def single(i):
            pkg.reproject(im_in[i % n_res], im_out[i % n_res][0], ns, wl["interp"], rot, post=post, stream=stream)

    if timed_region_ms:  # the headline workload: the launches of the timed region itself
        b_avg, b_min = sum(timed_region_ms) / len(timed_region_ms), min(timed_region_ms)
    else:
        for i in range(12):  # table builds; ~20 ms of this kernel so that the clock has settled
            batched(i)
        torch.cuda.synchronize()
        b_avg, b_min = time_launches(torch, stream, batched, 32)
    launch_bytes = (size * size + out_size * out_size) * c * 4
    frame_bytes = launch_bytes * (len(faces) if faces else 1)

    def single_on(i, st):
        if faces:
            pkg.reproject_multi(im_in[i % n_res], im_out[i % n_res], ns, wl["interp"], rots, post=post, stream=st)
        else:
            pkg.reproject(im_in[i % n_res], im_out[i % n_res][0], ns, wl["interp"], rot, post=post, stream=st)

    def single_launch_figures():
        """Single-frame launches — the call the reference's worker makes once per file (src/main.cpp:597): with the geometry
        cache (the first launch of the geometry fills it, the timed ones read it), dealt alternately to two streams (what
        lrp_context does with consecutive images: the tail of one launch overlaps the head of the next; wall time per launch
        between a fork and a join on `stream`), on one stream measured the same way, and with every launch computing its own
        coordinates (lrp_debug_set geo_cache 0)."""
        for i in range(16):
            single(i)
        torch.cuda.synchronize()
        s_avg, s_min = time_launches(torch, stream, single, 64)
        side = torch.cuda.Stream(device=stream.device)

        def two_stream_us(reps=64):
            best = None
            for _ in range(3):
                e0, e1, ej = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event()
                e0.record(stream)
                side.wait_event(e0)
                for i in range(reps):
                    single_on(i, side if i & 1 else stream)
                ej.record(side)
                stream.wait_event(ej)
                e1.record(stream)
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / reps
                best = us if best is None else min(best, us)
            return best

        for i in range(8):
            single_on(i, side if i & 1 else stream)
        torch.cuda.synchronize()
        two_us = two_stream_us()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for i in range(64):
            single_on(i, stream)
        e1.record(stream)
        torch.cuda.synchronize()
        one_stream_wall_us = e0.elapsed_time(e1) * 1e3 / 64
        prev_geo = pkg.debug_set("geo_cache", 0)
        try:  # (the switch is process-wide: whatever happens in here, the launches after it run the default again)
            for i in range(8):
                single(i)
            torch.cuda.synchronize()
            u_avg, _u_min = time_launches(torch, stream, single, 32)
        finally:
            pkg.debug_set("geo_cache", prev_geo)
        return {
            "single_launch_us": s_avg * 1e3,
            "single_launch_us_min": s_min * 1e3,
            "single_launch_frac": frame_bytes / (s_avg * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "single_launch_us_two_streams": two_us,
            "single_launch_frac_two_streams": frame_bytes / (two_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
            "single_launch_us_one_stream_wall": one_stream_wall_us,
            "single_launch_us_uncached": u_avg * 1e3,
            "single_launch_frac_uncached": frame_bytes / (u_avg * 1e-3) / 1e9 / HBM_PEAK_GBS,
        }

    singles = single_launch_figures() if single_legs else {}
    # (inW*inH + outW*outH)*C*4 per launch that reads the source; a cubemap is six such launches
    read_bytes = size * size * c * 4 * (len(faces) if faces else 1)
    algo = frame_bytes * nb
    achieved = algo / (b_avg * 1e-3) / 1e9
    traffic_b, traffic_s = measured_traffic(name) if size == wl["size"] else (None, None)
    if faces:  # (a cubemap "frame" is its own launch shape: six launches)
        traffic_b = traffic_s
    hbm_bytes = (traffic_b or {}).get("hbm_bytes_per_launch")
    out = {
        "bound": "hbm",
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "frac_read_only": read_bytes * nb / (b_avg * 1e-3) / 1e9 / HBM_PEAK_GBS,
        # the bytes the PMC counters saw cross the HBM interface / time / peak: what the memory system actually sustains
        # (below frac whenever the view does not look at the whole source)
        "frac_measured_hbm": (hbm_bytes / (b_avg * 1e-3) / 1e9 / HBM_PEAK_GBS) if hbm_bytes else None,
        # PMC bytes of one launch as timed here (rocprofv3 FETCH_SIZE / WRITE_SIZE passes over that launch shape; null when the
        # traffic file was measured on other kernel sources)
        "traffic": hbm_bytes or None,
        "traffic_detail": {"batched_launch": traffic_b, "single_launch": traffic_s, "file": TRAFFIC_FILE},
        "kernel": "six launches of reproject_bicubic_win_kernel (LDS window) over one resident source" if faces else KERNEL_NAMES[wl["interp"]],
        "workload": name,
        "kernel_ms_avg": b_avg,
        "kernel_ms_min": b_min,
        "kernel_launches_timed": len(timed_region_ms) if timed_region_ms else 32,
        "timed": "every 16-frame launch of the timed region" if timed_region_ms else "32 launches after 12 of warm-up",
        "frames_per_launch": nb,
        "us_per_frame": b_avg * 1e3 / nb,
        "algorithmic_bytes_per_launch": algo,
        **singles,
    }
    if faces:
        # the source read ONCE + the six faces written: what a cubemap has to move (SURVEY 8d's figure counts the whole source per face)
        once = size * size * c * 4 + len(faces) * out_size * out_size * c * 4
        out["frac_source_once"] = once / (b_avg * 1e-3) / 1e9 / HBM_PEAK_GBS
        # (`frac` counts the whole source once per face launch as SURVEY 8d prescribes and exceeds 1 — a 90-degree face looks at a sixth
        # of the source; frac_source_once is the honest fraction and the one the compact line carries for this workload)
    return out


def golden_batch_digest(workload, total_images):
    """sha256 over the committed per-image checksums (tests/golden/fullframe_golden.json, written by the oracle in
    the build container) of the first `total_images` images of the batch, or None if there is no fixture."""
    try:
        with open(os.path.join(ROOT, "tests", "golden", "fullframe_golden.json")) as f:
            sums = json.load(f)["bench_batch"][workload]["checksums"]
    except (OSError, ValueError, KeyError):
        return None
    if total_images > len(sums):
        return None
    return hashlib.sha256(",".join(sums[:total_images]).encode()).hexdigest()


DUMP_SAMPLE_BYTES = 48 << 20  # the per-image pixel samples; the crop of image 0 adds at most 256^2 pixels
DUMP_CROP = 256
DUMP_SEED = 0x5EED


def dump_outputs(torch, dsts, n_images, total_images, dist, rank, out_dir):
    """What the last timed step rendered, as .npy files in `out_dir` (rank 0 writes; float32): the same seeded sample of pixel
    positions of every image of the batch, in image order over all ranks (outputs_sample: images x pixels x channels; image k of
    a rank's block is in resident destination k % len(dsts)), the sampled positions (pixel_index, row-major, float64) and the
    central DUMP_CROP^2 window of image 0 at full resolution (image0_crop).  A frame's output is 256 MiB: the sample keeps a run
    under 64 MB whatever the batch."""
    import numpy as np

    h, w, c = dsts[0].shape
    per_image = max(1, min(h * w, DUMP_SAMPLE_BYTES // (total_images * c * 4)))
    rng = np.random.default_rng(DUMP_SEED)
    pix = np.arange(h * w) if per_image == h * w else np.sort(rng.choice(h * w, per_image, replace=False))
    idx = torch.from_numpy(pix).to(dsts[0].device)
    slots = [d.view(-1, c).index_select(0, idx).cpu().numpy() for d in dsts[:n_images]]
    sample = np.stack([slots[k % len(slots)] for k in range(n_images)]) if n_images else np.empty((0, per_image, c), np.float32)
    blocks = [sample]
    if dist is not None:
        blocks = [None] * dist.get_world_size()
        dist.all_gather_object(blocks, sample)
    if rank != 0:
        return
    ch, cw = min(DUMP_CROP, h), min(DUMP_CROP, w)
    y0, x0 = (h - ch) // 2, (w - cw) // 2
    crop = dsts[0][y0:y0 + ch, x0:x0 + cw].cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "outputs_sample.npy"), np.concatenate(blocks).astype(np.float32, copy=False))
    np.save(os.path.join(out_dir, "pixel_index.npy"), pix.astype(np.float64))
    np.save(os.path.join(out_dir, "image0_crop.npy"), crop.astype(np.float32, copy=False))


# ---- the line the driver reads --------------------------------------------------------------------------------------
# bench.py's LAST stdout line is ONE compact JSON object (the contract keys + the roofline and cpu_baseline objects + one
# {frac, us_per_frame} pair per secondary workload); everything else that is measured — notes, traffic detail, two-stream and
# uncached figures, per-rank times, the staged rates — goes to the detail file (--detail-file, default bench_detail.json).
# Round 5's single line had grown to 24.7 KB and the driver could no longer read it.
COMPACT_LIMIT = 4000
ROOFLINE_KEYS = ("bound", "achieved", "peak", "unit", "frac", "frac_read_only", "frac_measured_hbm", "traffic", "kernel", "kernel_ms_avg",
                 "frames_per_launch", "algorithmic_bytes_per_launch", "single_launch_us", "single_launch_frac",
                 "single_launch_us_two_streams", "single_launch_frac_two_streams")
CPU_KEYS = ("value", "unit", "cores", "kind", "single_thread_value", "cpu_model", "sample")
TOP_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
            "data", "config", "roofline", "cpu_baseline", "outputs_match_golden", "secondary", "detail_file")


def _short(v, digits=6):
    """Floats to `digits` significant digits (the line is a report, the detail file keeps every bit)."""
    if isinstance(v, float):
        if v != v or v in (float("inf"), float("-inf")):
            return None  # (never a NaN / Infinity token on the driver's line)
        return float(f"{v:.{digits}g}")
    return v


def compact_line(detail, detail_file=None):
    """The driver's line from the full result: a pure function (tests/test_tools.py feeds it a canned result)."""
    cfg = detail.get("config") or {}
    out = {k: _short(detail.get(k)) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                                "scaling", "vs_baseline", "dtype", "data")}
    out["config"] = {k: cfg[k] for k in ("workload", "images_per_step", "images_per_gpu_per_step", "frames_per_launch", "parallelism")
                     if k in cfg}
    roof = detail.get("roofline") or {}
    out["roofline"] = {k: _short(roof.get(k)) for k in ROOFLINE_KEYS if k in roof}
    cpu = detail.get("cpu_baseline")
    if cpu:
        out["cpu_baseline"] = {k: _short(cpu.get(k)) for k in CPU_KEYS if k in cpu}
        out["cpu_baseline"]["sample"] = str(cpu.get("sample", ""))[:200]
    out["outputs_match_golden"] = detail.get("outputs_match_golden")
    out["secondary"] = {name: {"frac": _short(r.get("frac_source_once", r.get("frac")), 4), "us_per_frame": _short(r.get("us_per_frame"), 4)}
                        for name, r in (detail.get("secondary") or {}).items()}
    if detail_file:
        out["detail_file"] = detail_file
    line = json.dumps(out, separators=(",", ":"))
    assert len(line) <= COMPACT_LIMIT, f"bench.py: the driver's line grew to {len(line)} bytes (limit {COMPACT_LIMIT})"
    return line


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.force_dist and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_under_torchrun(args))  # (one rank under the launcher; nothing has touched the GPU yet)
    if args.gpus != world:
        if "WORLD_SIZE" in os.environ or args.gpus < 1:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch with python -m "
                             f"torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 "
                             f"--master-port P bench.py --gpus {args.gpus} ...")
        sys.exit(relaunch_under_torchrun(args))

    import torch

    pkg = importlib.import_module("image-lens-reproject_amd")
    sharding = importlib.import_module("image-lens-reproject_amd.sharding")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    dev_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.dist_backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend="gloo")
    dev = torch.device("cuda", dev_index)

    wl = dict(WORKLOADS[args.workload])
    size = args.size or wl["size"]
    c = wl["channels"]
    lin, lout = make_lens(pkg, wl["in_lens"], size, size), make_lens(pkg, wl["out_lens"], size, size)
    rot = make_rot(pkg, wl["rot"])

    # this rank's block of the sorted image list
    if args.scaling == "strong":
        first, last = sharding.my_block(args.batch, world, rank)
        total_images = args.batch
    else:
        first, last = rank * args.batch, (rank + 1) * args.batch
        total_images = args.batch * world
    shard = list(range(first, last))
    if args.steps <= 0:
        # 20 steps of a 256-image shard are 0.5 s; a rank of an 8-GPU job renders 32 images per step (3.3 ms): more steps, so
        # that barrier skew and launch latency do not dominate what the driver's clock sees
        args.steps = 20 if len(shard) >= 64 else min(160, 20 * -(-64 // max(len(shard), 1)))

    # resident frames: the whole shard when it fits (288 GB of HBM: 256 x 2 x 256 MiB = 128 GiB), else a
    # ring of at least 16 pairs — far beyond the 256 MiB Infinity Cache either way
    frame_bytes = size * size * c * 4
    free_b, _total_b = torch.cuda.mem_get_info(dev)
    fit = max(1, int(0.70 * free_b / (2 * frame_bytes)))
    n_res = args.distinct if args.distinct > 0 else min(max(len(shard), 1), fit)
    n_res = max(1, min(n_res, max(len(shard), 1)))
    if wl.get("faces"):
        raise SystemExit("bench.py: the cubemap is a secondary workload (six launches per frame), not a batch headline")
    srcs, dsts = [], []
    for k in range(n_res):
        s = torch.empty((size, size, c), dtype=torch.float32, device=dev)
        pkg.synth_fill(s, size, size, c, 0x5EED0000 + (shard[k] if shard else 0), wl.get("depth", -1))
        srcs.append(s)
        dsts.append(torch.empty((size, size, c), dtype=torch.float32, device=dev))
    post = wl.get("post")
    im_in = [pkg.Image(lin, size, size, c, s) for s in srcs]
    im_out = [pkg.Image(lout, size, size, c, d) for d in dsts]
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(1, args.streams))]
    torch.cuda.synchronize()

    batch_in = [im_in[k % n_res] for k in range(len(shard))]
    batch_out = [im_out[k % n_res] for k in range(len(shard))]
    launches_per_step = len(shard) if args.per_frame_launches else -(-len(shard) // FRAMES_PER_LAUNCH)
    # the frames of a step share one geometry: one launch per 16 frames, descriptors marshalled once
    groups = [pkg.PreparedBatch(batch_in[k:k + FRAMES_PER_LAUNCH], batch_out[k:k + FRAMES_PER_LAUNCH], wl.get("ns", 1), wl["interp"], rot, post=post)
              for k in range(0, len(shard), FRAMES_PER_LAUNCH)] if not args.per_frame_launches else []
    # HIP events around every launch of the timed region, on the stream it is launched on (roofline.achieved)
    events = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in groups]
              for _ in range(args.steps)]

    def step(timed=None):
        if args.per_frame_launches:
            for k in range(len(shard)):
                pkg.reproject(batch_in[k], batch_out[k], wl.get("ns", 1), wl["interp"], rot, post=post, stream=streams[k % len(streams)])
            return
        for gi, g in enumerate(groups):
            if timed is not None:
                events[timed][gi][0].record(streams[0])
            g.launch(stream=streams[0])
            if timed is not None:
                events[timed][gi][1].record(streams[0])

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # N > 1: the first collective of a process group sets the communicator up (RCCL: seconds, the GPU idle meanwhile).  It runs
    # HERE, in front of the settling launches, so that the barrier in front of the timed region is a fast one on a GPU that is
    # at its loaded clock — a first launch after idle is 10-25 % slower, and at 8 GPUs the whole timed region is ~60 ms.
    barrier()
    t_settle = time.perf_counter()
    while time.perf_counter() - t_settle < args.settle_seconds:
        step()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for s_i in range(args.steps):
        step(s_i)
    barrier()
    elapsed_rank = time.perf_counter() - t0
    # device time of this rank's timed launches alone (first event to last event on its stream): what the rank would need
    # without the barriers; the difference to elapsed_rank is host / barrier time
    busy_rank = events[0][0][0].elapsed_time(events[-1][-1][1]) * 1e-3 if events and events[0] else None
    per_rank = [(elapsed_rank, busy_rank)]
    if dist is not None:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, (elapsed_rank, busy_rank))
    elapsed = sharding.max_over_ranks(elapsed_rank, dist, dev if args.dist_backend == "nccl" else None, always=args.force_dist)
    # full 16-frame launches of the timed region (a shard's last launch may hold fewer frames)
    timed_ms = [a.elapsed_time(b) for per_step in events for (a, b), g in zip(per_step, groups) if g._n == FRAMES_PER_LAUNCH]
    if args.dump_outputs:  # (before anything else renders into the destinations)
        dump_outputs(torch, dsts, len(shard), total_images, dist, rank, args.dump_outputs)

    # --full: per-image checksums of what the timed steps rendered (only when every image of the shard has its
    # own resident destination), gathered in image order — a reporting step, not on the data path
    all_sums, digest = [None], None
    if args.full or args.checksums_file:
        sums = pkg.checksums(dsts[: len(shard)]) if shard and n_res >= len(shard) else None
        all_sums = [sums]
        if dist is not None:
            all_sums = [None] * world
            dist.all_gather_object(all_sums, sums)
    if all(s is not None for s in all_sums):
        flat = [v for s in all_sums for v in s]
        digest = hashlib.sha256(",".join(f"{v:016x}" for v in flat).encode()).hexdigest()
        if rank == 0 and args.checksums_file:
            with open(args.checksums_file, "w") as f:
                json.dump({"images": total_images, "n_gpus": world, "checksums": [f"{v:016x}" for v in flat]}, f)

    bad_pixels = False
    # Without --full a run reports the timed region only.  N > 1: rank 0 reports the timed region only and the other ranks are
    # released at once (the single-launch legs and the secondary workloads are N = 1 measurements: ~15 s during which seven GPUs
    # would sit in a barrier); --full-legs overrides.
    full_legs = (world == 1 and args.full) or args.full_legs
    if args.secondary is None:
        args.secondary = DEFAULT_SECONDARY if full_legs else ""
    if args.detail_file is None:
        args.detail_file = "bench_detail.json" if args.full else ""
    if rank == 0:
        res = min(n_res, 64)
        # the headline kernel's figures come from the launches of the timed region; only --full times launches of its own
        # when the region holds fewer than four full 16-frame launches
        region_ms = timed_ms if len(timed_ms) >= 4 or (timed_ms and not args.full) else None
        roof = kernel_figures(torch, pkg, wl, size, srcs[:res], [[d] for d in dsts[:res]], streams[0], args.workload,
                              timed_region_ms=region_ms, single_legs=full_legs) if region_ms or args.full else None
        # (the un-fused IEEE arithmetic of the reference makes this kernel VALU-bound, not HBM-bound — DESIGN.md section 5;
        # frac is algorithmic bytes / kernel time / 8 TB/s as the contract asks)
        secondary = {}
        for name in [n for n in args.secondary.split(",") if n and n != args.workload]:
            w2 = WORKLOADS[name]
            size2 = w2["size"] * size // wl["size"]  # (--size scales every workload alike: tests)
            if (w2["channels"] == c and size2 == size and not w2.get("faces") and w2.get("depth", -1) == wl.get("depth", -1) and
                    w2.get("out_size", w2["size"]) == w2["size"] and wl.get("out_size", wl["size"]) == wl["size"]):
                secondary[name] = kernel_figures(torch, pkg, w2, size, srcs[:res], [[d] for d in dsts[:res]], streams[0], name)
            else:  # its own resident frames: 32 pairs (4 panoramas + cubemaps for configs[4]), far beyond the Infinity Cache
                s2, d2 = resident_frames(torch, pkg, w2, size2, 4 if w2.get("faces") else min(32, max(res, 1)), dev, 0x5EED1000)
                secondary[name] = kernel_figures(torch, pkg, w2, size2, s2, d2, streams[0], name)
                del s2, d2
                torch.cuda.empty_cache()
        value = total_images * size * size * args.steps / elapsed / 1e6
        golden = (golden_batch_digest(args.workload, total_images) if args.full and size == wl["size"] and args.scaling == "strong"
                  else None)
        out = {
            "metric": f"Mpix/s reprojected ({'4K' if size == 4096 else size} {'RGBA' if c == 4 else f'{c}-channel'} float, "
                      f"{INTERP_NAMES[wl['interp']]})",
            "value": value,
            "unit": "Mpix/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "timed_region_s": elapsed,
            # one entry per rank: wall seconds between its barriers, device seconds of its own launches; skew = slowest - fastest
            "per_rank_elapsed_s": [e for e, _b in per_rank],
            "per_rank_device_busy_s": [b for _e, b in per_rank],
            "rank_skew_s": max(e for e, _b in per_rank) - min(e for e, _b in per_rank),
            "settle_seconds": args.settle_seconds,
            "dist": (f"{args.dist_backend} process group, world size {world}" + (" (--force-dist)" if args.force_dist else "")) if dist is not None else None,
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{args.workload}: {size}x{size}x{c} f32 -> {size}x{size}x{c}, "
                            f"{wl['in_lens']}->{wl['out_lens']}, interp={wl['interp']}, num_samples=1",
                "images_per_step": total_images,
                "images_per_gpu_per_step": len(shard),
                "resident_distinct_frames_per_gpu": n_res,
                "streams": len(streams),
                "launches_per_step_per_gpu": launches_per_step,
                "frames_per_launch": 1 if args.per_frame_launches else FRAMES_PER_LAUNCH,
                "parallelism": f"image-sharded x{world} (static blocks of the sorted list), no collective",
            },
            "outputs_digest": digest,
            # the same digest from the per-image checksums the ORACLE produced in the build container (committed fixture)
            "outputs_digest_golden": golden,
            "outputs_match_golden": (digest == golden) if (digest and golden) else None,
            "roofline": roof,
            "secondary": secondary,
        }
        if world == 1 and args.full and not args.no_staged:
            out["staged"] = staged_rates()
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(pkg, wl, args.cpu_seconds)
        detail_file = None
        if args.detail_file:
            try:
                with open(os.path.join(ROOT, args.detail_file) if not os.path.isabs(args.detail_file) else args.detail_file, "w") as f:
                    json.dump(out, f, indent=1)
                detail_file = args.detail_file
            except OSError as e:  # (a read-only checkout: the compact line is still the result)
                print(f"bench.py: could not write {args.detail_file}: {e}", file=sys.stderr, flush=True)
        print(compact_line(out, detail_file), flush=True)  # the LAST stdout line: what the driver reads
        if digest and golden and digest != golden:
            print("bench.py: the rendered batch differs from the committed oracle checksums (tests/golden/fullframe_golden.json): "
                  "the number above was measured on WRONG pixels", file=sys.stderr, flush=True)
            bad_pixels = True
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if bad_pixels:
        sys.exit(3)


if __name__ == "__main__":
    main()
