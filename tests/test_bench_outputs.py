"""bench.py's plain run and --dump-outputs.

A plain `bench.py --gpus 1 --steps K --warmup W` times K steps and prints the line: none of the --full legs (single launches,
secondary workloads, host-buffer rates, CPU baseline, oracle checksums, detail file).  --dump-outputs DIR writes what the last
timed step rendered: a seeded sample of pixel positions of every image of the batch and a crop of image 0, float32, under
64 MB, identical from run to run.  CPU: the sampler on host tensors.  -m gpu: two plain runs, against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SIZE, BATCH = 512, 24


def _dump_files(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d)) if n.endswith(".npy")}


def test_dump_outputs_is_a_seeded_sample_in_image_order_under_64_mb(tmp_path):
    """Two resident destinations serving a 256-image batch of 1024^2 x 5 frames (image k is in destination k % 2): every row of
    the sample holds its image's pixels at the recorded positions, the files stay under 64 MB, and a second dump is identical."""
    import torch

    sys.path.insert(0, ROOT)
    import bench

    h = w = 1024
    c, images = 5, 256
    dsts = [torch.arange(h * w * c, dtype=torch.float32).reshape(h, w, c) + 0.5 * k for k in range(2)]
    for name in ("a", "b"):
        bench.dump_outputs(torch, dsts, images, images, None, 0, str(tmp_path / name))
    a, b = _dump_files(tmp_path / "a"), _dump_files(tmp_path / "b")
    assert set(a) == {"outputs_sample", "pixel_index", "image0_crop"}
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in a) < 64 * 10**6
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
    pix = a["pixel_index"].astype(np.int64)
    sample = a["outputs_sample"]
    assert sample.shape == (images, len(pix), c) and len(np.unique(pix)) == len(pix) > 1000
    for k in (0, 1, 2, images - 1):
        assert np.array_equal(sample[k], dsts[k % 2].view(-1, c)[torch.from_numpy(pix)].numpy()), k
    y0 = x0 = (h - bench.DUMP_CROP) // 2
    assert np.array_equal(a["image0_crop"], dsts[0][y0:y0 + bench.DUMP_CROP, x0:x0 + bench.DUMP_CROP].numpy())


def plain_run(tmp_path, tag):
    dump = tmp_path / f"dump_{tag}"
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(BATCH), "--size", str(SIZE), "--settle-seconds", "0",
            "--dump-outputs", str(dump)]
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.rstrip("\n").splitlines()[-1]), _dump_files(dump)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_oracles_pixels(lrp, oracle, torch_cuda, tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    rec, got = plain_run(tmp_path, "a")
    rec2, got2 = plain_run(tmp_path, "b")
    for r in (rec, rec2):
        assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
        assert r["unit"] == "Mpix/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
        assert "cpu_baseline" not in r and "detail_file" not in r and r["secondary"] == {} and r["outputs_match_golden"] is None
        assert "single_launch_us" not in r["roofline"]
    assert set(got) == set(got2) == {"outputs_sample", "pixel_index", "image0_crop"}
    for n in got:
        assert np.array_equal(got[n], got2[n]), n
    wl = bench.WORKLOADS["fisheye_to_rect_bicubic"]
    lin, lout = bench.make_lens(lrp, wl["in_lens"], SIZE, SIZE), bench.make_lens(lrp, wl["out_lens"], SIZE, SIZE)
    pix = got["pixel_index"].astype(np.int64)
    assert got["outputs_sample"].shape == (BATCH, len(pix), 4)
    for i in (0, BATCH - 1):
        want = oracle.reproject(lin, oracle.synth_frame(SIZE, SIZE, 4, 0x5EED0000 + i), lout, SIZE, SIZE, 1, wl["interp"], None)
        assert np.array_equal(got["outputs_sample"][i].view(np.uint32), want.reshape(-1, 4)[pix].view(np.uint32)), f"image {i}"
        if i == 0:
            y0 = x0 = (SIZE - bench.DUMP_CROP) // 2
            crop = want[y0:y0 + bench.DUMP_CROP, x0:x0 + bench.DUMP_CROP]
            assert np.array_equal(got["image0_crop"].view(np.uint32), crop.view(np.uint32))
