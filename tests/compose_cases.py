"""The cases of the compose tests (include/lrp.h "compose"), shared by tests/test_compose.py (CPU: every case discriminates, by
the coverage model) and tests/test_gpu_compose.py (the HIP launch against the composition, by the definition, of what the
existing reproject() and coverage() calls deliver).

A case: the output lens and size and a list of sources (lens name of tests/coverage_cases.py, size, rotation in degrees or
None); all sources of a case are of one source mode.  expect() is the definition in numpy float32 — a select for FIRST, adds
and one division for MEAN, and for FEATHER the weights from the coordinates the CPU models deliver."""
import numpy as np

import coverage_cases as cc

FIRST, MEAN, FEATHER = 0, 1, 2
MODES = (FIRST, MEAN, FEATHER)
MODE_NAMES = {FIRST: "first", MEAN: "mean", FEATHER: "feather"}


def _case(name, out, out_size, sources):
    return dict(name=name, out=out, out_size=out_size, sources=sources)


def _pan(deg):
    return (float(deg), 0.0, 0.0)


# Overlap cases: pixels with k = 0, k = 1 and k >= 2 are each at least 5 % of the output, and FIRST in reversed source order
# differs from FIRST in at least 1 % of the pixels (tests/test_compose.py checks both on the CPU).
OVERLAP_CASES = [
    # a rig of three overlapping rectilinear cameras into a panorama; one of them with another size and focal length
    _case("rect3_pano", "eqr_full", (96, 48), [("rect18", (64, 48), _pan(0)), ("rect12", (48, 32), _pan(40)), ("rect18", (64, 48), _pan(80))]),
    # two 180 degree fisheyes.  Back to back (pans 0 and 180) they are complementary: a folding source covers at most the
    # hemisphere in front of it (vz < 0), so k is 1 everywhere.  130 degrees apart the hemispheres overlap and leave a lune uncovered;
    # the 64 x 40 frames cut the image circle at the poles.
    _case("fisheye2_pano", "eqr_full", (80, 48), [("eqd_pi", (64, 40), _pan(0)), ("eqd_pi", (64, 40), _pan(130))]),
    # two partial panoramas (clamped in x and y) shifted in pan, into an 18 mm view.  Shifted in pan alone they leave 2.7 % of
    # the view uncovered (two thin strips above and below); with 8 degrees of pitch as well the model gives 11.9 / 54.2 / 33.9 %.
    _case("part2_rect", "rect18", (80, 48), [("eqr_part", (64, 32), (-35.0, 8.0, 0.0)), ("eqr_part", (64, 32), (35.0, 8.0, 0.0))]),
    # two wrapping bands of latitude at different pitch: in_y alone decides, the weight is dy alone
    _case("band2_pano", "eqr_full", (80, 48), [("eqr_band", (64, 32), (0.0, -22.0, 0.0)), ("eqr_band", (64, 24), (0.0, 22.0, 0.0))]),
    # the extension lenses (their bits on)
    _case("eqs2_pano", "eqr_full", (80, 48), [("eqs", (64, 48), _pan(-35)), ("eqs", (48, 48), _pan(35))]),
    _case("stg2_pano", "eqr_full", (80, 48), [("stg", (64, 48), _pan(-35)), ("stg", (48, 48), _pan(35))]),
]

# The cube: six 90 x 90 degree faces (18 mm on a 36 mm square sensor) into a full panorama.  Rounding at the seams decides how
# many pixels no face or two faces cover; the model is the authority (CUBE_SEAMS, asserted by tests/test_compose.py and by the GPU).
CUBE_ROTATIONS = [_pan(0), _pan(90), _pan(180), _pan(270), (0.0, 90.0, 0.0), (0.0, -90.0, 0.0)]


def cube_case(face, out_w, out_h):
    return _case(f"cube{face}_pano", "eqr_full", (out_w, out_h), [("rect18", (face, face), r) for r in CUBE_ROTATIONS])


CUBE = cube_case(32, 128, 64)
CUBE_MID = cube_case(512, 2048, 1024)
# pixels of CUBE with k == 0 and with k >= 2, by the model
CUBE_SEAMS = dict(k0=14, k2=110)

CASES = OVERLAP_CASES + [CUBE]


def lenses(lrp, case):
    ow, oh = case["out_size"]
    return cc.lens(lrp, case["out"], ow, oh), [cc.lens(lrp, name, w, h) for name, (w, h), _ in case["sources"]]


def wraps(lens_name):
    return lens_name in ("eqr_band", "eqr_full")


def cell_case(out_name, src_name, src_size):
    """The three sources of a cell of the 30-cell sweep (tests/coverage_cases.py cells()): two that overlap and one at a general
    rotation of coverage_cases.CELL_ROTATIONS; one of another size.  The fisheye targets look along +z, the others along -z:
    the overlapping pair is turned to face the target."""
    w, h = src_size
    base = 180.0 if out_name in ("eqd_pi", "eqs", "stg") else 0.0
    apart = 55.0 if src_name in ("eqs", "stg", "eqr_band") else 13.0  # (the wide sources further apart: a pixel of every k in most cells)
    return _case(f"{out_name}<-{src_name}", out_name, (80, 48),
                 [(src_name, (w, h), _pan(base - apart)), (src_name, (w - 16, h - 8), (base + apart, apart - 5.0, 0.0)), (src_name, (w, h), cc.CELL_ROTATIONS[1])])


def feather_weight(sxy, in_w, in_h, wrapping):
    """w_i of include/lrp.h "compose" from the sampler coordinates sxy (..., 2), binary32."""
    half, floor = np.float32(0.5), np.float32(2.0 ** -10)
    sx, sy = sxy[..., 0].astype(np.float32), sxy[..., 1].astype(np.float32)
    with np.errstate(invalid="ignore"):
        dy = np.minimum(sy + half, (np.float32(in_h) - half) - sy)
        m = dy if wrapping else np.minimum(np.minimum(sx + half, (np.float32(in_w) - half) - sx), dy)
        return np.where(m < floor, floor, m).astype(np.float32)


def expect(mode, renders, planes, weights=None):
    """The composed image (H, W, C) float32 and k (H, W) uint8 by the definition: renders[i] is source i reprojected alone
    (num_samples 1, no post), planes[i] its coverage plane, weights[i] its feather_weight() (FEATHER only)."""
    covered = [p > 0 for p in planes]
    k = np.sum(covered, axis=0).astype(np.uint8)
    zero = np.zeros_like(renders[0], dtype=np.float32)
    with np.errstate(all="ignore"):
        if mode == FIRST:
            out, taken = zero.copy(), np.zeros(k.shape, dtype=bool)
            for r, c in zip(renders, covered):
                sel = c & ~taken
                out[sel] = r[sel]
                taken |= c
            return out, k
        acc, wsum = zero.copy(), np.zeros(k.shape, dtype=np.float32)
        for i, (r, c) in enumerate(zip(renders, covered)):
            if mode == MEAN:
                acc = np.where(c[..., None], acc + r, acc)
            else:
                w = weights[i]
                acc = np.where(c[..., None], acc + w[..., None] * r, acc)
                wsum = np.where(c, wsum + w, wsum)
        div = k.astype(np.float32) if mode == MEAN else wsum
        out = np.where((k > 0)[..., None], acc / div[..., None], np.float32(0.0)).astype(np.float32)
    return out, k
