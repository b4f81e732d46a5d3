"""The cases of the supersampled compose tests (include/lrp.h "compose, supersampled"), shared by tests/test_compose_ss.py (CPU:
the model is the definition, and every case discriminates) and tests/test_gpu_compose_ss.py (the HIP launch against the model
of tests/compose_ss_model.py, byte for byte).

The geometries are those of tests/compose_cases.py.  What a supersampled case has to show that a num_samples == 1 one cannot:
pixels whose sub-samples are only partly covered (0 < m < n * n: the division by m, not n * n), and pixels whose sub-samples
are covered by different sets of sources (coverage decided per sub-sample, not per pixel).  The conditions below are asserted
on the CPU, with the coverage model, by tests/test_compose_ss.py."""
import numpy as np

import cases
import compose_cases as cs
import coverage_model as model

# ---- the overlap cases and the n at which they are used
# rect3_pano, part2_rect, band2_pano, stg2_pano at every n of 2, 3, 4: at least PARTIAL_MIN of the pixels have 0 < m < n * n
# (measured minimum 0.8 %) and at least SET_DIFFERS_MIN a covering-source set that differs among their sub-samples (1.8 %).
# eqs2_pano does NOT discriminate at n = 2 and 3: the boundaries of its sources fall between pixel columns (0.0 %); at n = 4 it
# does (5 %), and there alone it is used.  (fisheye2_pano is just below both bounds at n = 2 — 0.52 % and 0.99 % — and is not used.)
PARTIAL_MIN = 0.005
SET_DIFFERS_MIN = 0.01
# every cell of compose_cases.cell_case(): the covering set differs among the sub-samples of at least CELL_SET_DIFFERS_MIN of the
# pixels, at n = 2 and 3 (measured minimum 0.68 %, at n = 2)
CELL_SET_DIFFERS_MIN = 0.005

_BY_NAME = {c["name"]: c for c in cs.OVERLAP_CASES}
DISCRIMINATING = [(_BY_NAME[name], n) for name in ("rect3_pano", "part2_rect", "band2_pano", "stg2_pano") for n in (2, 3, 4)] + [(_BY_NAME["eqs2_pano"], 4)]
NOT_DISCRIMINATING = [(_BY_NAME["eqs2_pano"], 2), (_BY_NAME["eqs2_pano"], 3)]
# the n beyond those the coverage tests pin (a loop count of its own kind: odd, and the largest): the GPU test runs every case of
# DISCRIMINATING's geometries at these too
LARGE_N = (5, 15)
CELL_N = (2, 3)

# The cube (compose_cases.CUBE: six 32 x 32 faces into 128 x 64) at n = 2, by the model: pixels with no covered sub-sample (the
# 14 of n = 1 are binary32 cracks at the seams; a pixel with four sub-samples is uncovered only if all four fall into one),
# pixels with some but not all sub-samples covered, and pixels that more than one face covers some sub-sample of.
CUBE_SEAMS_N2 = dict(m0=0, partial=32, count2=256)

FOLDING = ("rect18", "rect12", "rect35", "eqd_pi", "eqd_narrow", "eqd_15pi", "eqs", "stg")  # sources that fold a ray through x / -z


def case_id(item):
    case, n = item
    return f"{case['name']}-n{n}"


def rotations(lrp, case):
    return [cases.rotation(lrp, deg) for _, _, deg in case["sources"]]


def sources(case, channels=4, seed=400, planted=False):
    """The noise sources of a case; without planted texels none is zero (+0.25), so that a zero pixel is an uncovered one."""
    noise = [cases.hash_noise(h, w, channels, seed + i, planted=planted) for i, (_, (w, h), _) in enumerate(case["sources"])]
    return noise if planted else [a + np.float32(0.25) for a in noise]  # (planted: untouched, an addition would lose the -0.0)


def sub_covered(lrp, case, n):
    """(n_src, H, W, n * n) bool: the coverage definition of include/lrp.h applied in numpy (binary32 comparisons, NaN false) to the
    coordinates and rotated z that coverage_model.coverage(detail=True) delivers per sub-sample, in the loop's order."""
    lout, lins = cs.lenses(lrp, case)
    ow, oh = case["out_size"]
    out = []
    for lin, (name, (w, h), deg) in zip(lins, case["sources"]):
        plane, sxy, vz = model.coverage(lin, w, h, lout, ow, oh, n, cases.rotation(lrp, deg), detail=True)
        sx, sy = sxy[..., 0], sxy[..., 1]
        with np.errstate(invalid="ignore"):
            front = (vz < np.float32(0.0)) if name in FOLDING else np.ones(sx.shape, bool)
            in_x = (sx == sx) if cs.wraps(name) else ((sx >= np.float32(-0.5)) & (sx <= np.float32(w) - np.float32(0.5)))
            in_y = (sy >= np.float32(-0.5)) & (sy <= np.float32(h) - np.float32(0.5))
        cov = front & in_x & in_y
        assert (cov.sum(axis=2) == plane).all(), "the numpy restatement against the model's own count"
        out.append(cov)
    return np.stack(out)


def planes(cov):
    """count, m of the definition from sub_covered()'s array."""
    kj = cov.sum(axis=0)  # (H, W, n * n)
    return cov.any(axis=3).sum(axis=0).astype(np.uint8), (kj > 0).sum(axis=2).astype(np.uint8)


def fractions(cov):
    """(share of pixels with 0 < m < n * n, share of pixels whose covering-source set differs among their sub-samples)."""
    n2 = cov.shape[3]
    _, m = planes(cov)
    bits = (cov * (1 << np.arange(cov.shape[0]))[:, None, None, None]).sum(axis=0)  # the covering set of every sub-sample
    differs = (bits != bits[..., :1]).any(axis=2)
    return float(((m > 0) & (m < n2)).mean()), float(differs.mean())
