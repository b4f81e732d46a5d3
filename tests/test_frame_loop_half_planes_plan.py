"""The mapping `half_block_planes` of tests/test_gpu_frame_loop_tier_dispatch.py is there for ONE block: a coefficient-tier
block whose planes fit per half only (`whole` clear), the only kind that runs the second precompute() of the coefficient tier's
frame loop (lrp_win_kernel.h coef_frames).  Whether it has such a block is a matter of the plan's thresholds and the lenses'
defaults, so it is checked here, on the CPU: the oracle's source coordinates of the mapping, cut into the kernel's 16 x 16
blocks (lanes and rows beyond the image hold the pixel they were clamped to), through the plan model of
tools/analysis/lds_conflict_census.py (win_plan_block for 16-byte texel slots: RGB / RGBA).

Asserted: of the nine blocks, coefficient tier with whole-block planes 2, with half-block planes 1, raw taps 1, nothing staged 5
— and in particular at least one block with half-block planes."""
import os
import sys

import numpy as np

import cases
import oracle_binding as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _blocks(sxy, ow, oh):
    nbx, nby = (ow + 15) // 16, (oh + 15) // 16
    ys, xs = np.minimum(np.arange(nby * 16), oh - 1), np.minimum(np.arange(nbx * 16), ow - 1)
    return sxy[ys][:, xs].reshape(nby, 16, nbx, 16, 2).transpose(0, 2, 1, 3, 4).reshape(-1, 16, 16, 2)


def test_half_block_planes_mapping_has_a_block_with_half_block_planes(lrp):
    sys.path.insert(0, os.path.join(ROOT, "tools", "analysis"))
    try:
        import lds_conflict_census as census
    finally:
        sys.path.pop(0)
    import test_gpu_frame_loop_tier_dispatch as gpu_test

    inp, (iw, ih), out, (ow, oh), deg = gpu_test.MAPPINGS["half_block_planes"]
    lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, ow, oh)[out]
    b = _blocks(oracle.source_coords(lin, iw, ih, lout, ow, oh, cases.rotation(lrp, deg)), ow, oh)
    sx, sy = b[..., 0], b[..., 1]
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(sx).all(axis=(1, 2)) & np.isfinite(sy).all(axis=(1, 2))
        sx0, sy0 = np.where(np.isfinite(sx), sx, 0.0), np.where(np.isfinite(sy), sy, 0.0)
        f1, f2 = np.float32(1.0), np.float32(2.0)
        exact = np.ones(sx.shape[0], dtype=bool)
        for s in (sx0, sy0):  # (taps_consecutive of lrp_kernel_common.h)
            t = np.trunc(s)
            exact &= ((np.trunc(s + f1) == t + f1) & (np.trunc(s + f2) == t + f2) & (np.abs(s) < 8388608.0)).all(axis=(1, 2))
        inside = ((sx0.min(axis=(1, 2)) >= 1.0) & (sx0.max(axis=(1, 2)) < np.float32(iw - 2)) &
                  (sy0.min(axis=(1, 2)) >= 1.0) & (sy0.max(axis=(1, 2)) < np.float32(ih - 2)))
    ix, iy = np.trunc(sx0).astype(np.int64), np.trunc(sy0).astype(np.int64)
    p = census.plan_blocks(ix, iy, finite & exact & inside, iw, ih)
    t = census.tiers(p, census.pitch_bw_or_1(p["bw"]))
    split = {"whole": int((t["coef"] & t["whole"]).sum()), "half": int((t["coef"] & ~t["whole"]).sum()),
             "raw": int((t["staged"] & ~t["coef"]).sum()), "unstaged": int((~t["staged"]).sum())}
    print(split)
    assert split["half"] >= 1, f"no coefficient block with half-block planes in this mapping any more: {split}"
    assert split == {"whole": 2, "half": 1, "raw": 1, "unstaged": 5}
