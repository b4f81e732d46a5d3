"""The cases of the coverage-plane tests (include/lrp.h "coverage"), shared by tests/test_coverage.py (CPU: the model against
the oracle's coordinates and a float64 restatement, and the rule that every case discriminates), tests/test_gpu_coverage.py
(the HIP plane against the model byte for byte) and tests/golden/make_coverage_golden.py.

CASES: geometries where the three conditions of the definition each decide something — both the count-0 and the count-n*n
pixels are between 5 % and 95 % of the plane and every n > 1 case has partial counts (checked on the CPU).
cells(): the 30 (output lens, source mode) cells of csrc/lrp_cells.h."""
import math

PI = math.pi
GENERAL = (30.0, -15.0, 5.0)  # pan, pitch, roll in degrees


def lens(lrp, name, w, h):
    L = lrp.LensInfo
    if name == "rect18":
        return L.rectilinear(18.0, 36.0, w, h)
    if name == "rect12":
        return L.rectilinear(12.0, 36.0, w, h)
    if name == "rect35":
        return L.rectilinear(35.0, 36.0, w, h)
    if name == "eqd_pi":
        return L.equidistant(PI)
    if name == "eqd_narrow":  # a 69 degree image circle
        return L.equidistant(1.2)
    if name == "eqd_15pi":
        return L.equidistant(1.5 * PI)
    if name == "eqs":
        return L.equisolid(12.5, 36.0, PI, w, h)
    if name == "stg":
        return L.stereographic(12.5, 36.0, w, h)
    if name == "eqr_full":
        return L.equirectangular()
    if name == "eqr_part":  # clamped in x and y
        return L.equirectangular(-1.0, 1.0, -0.5, 0.5)
    if name == "eqr_band":  # a full turn (wrapping in x) of a band of latitudes
        return L.equirectangular(-PI, PI, -0.5, 0.5)
    raise KeyError(name)


def _case(name, inp, in_size, out, out_size, deg, n):
    return dict(name=name, inp=inp, in_size=in_size, out=out, out_size=out_size, deg=deg, n=n)


CASES = [
    # BASELINE configs[3] in small: a rectilinear frame rendered into a full panorama — ghost (front) and smear (in_x, in_y)
    _case("rect_pano", "rect18", (64, 48), "eqr_full", (96, 48), None, 1),
    _case("rect_pano_rot_n2", "rect18", (64, 48), "eqr_full", (96, 48), GENERAL, 2),
    # a partial panorama as the source: the rectangle alone decides (an equirectangular source has no front test)
    _case("part_pano_rect_n3", "eqr_part", (64, 32), "rect18", (80, 48), (17.0, 6.0, 0.0), 3),
    # a wrapping source: in_y alone decides
    _case("band_pano_rect_n2", "eqr_band", (64, 32), "rect12", (80, 48), (0.0, 20.0, 10.0), 2),
    # a fisheye narrower than the view (a 180 degree fisheye would cover every pixel of a 12 mm view)
    _case("fisheye_rect_n2", "eqd_narrow", (64, 64), "rect12", (80, 48), None, 2),
    # passes the rectangle test everywhere: decided by front alone — the case that catches a missing vz test
    _case("eqd_eqd_front", "eqd_pi", (48, 48), "eqd_15pi", (64, 64), None, 1),
    _case("eqd_eqd_front_n4", "eqd_pi", (48, 48), "eqd_15pi", (64, 64), (10.0, 5.0, 0.0), 4),
    # the extension lenses as sources (front + image rectangle) and as a target with NaN rays (odd centre, beyond the circle)
    _case("eqs_pano_n2", "eqs", (64, 64), "eqr_full", (96, 48), GENERAL, 2),
    _case("stg_pano_n3", "stg", (64, 48), "eqr_full", (96, 48), None, 3),
    _case("rect_eqs_nan_n2", "rect12", (64, 48), "eqs", (49, 49), (160.0, 0.0, 0.0), 2),
    _case("tele_wide_n4", "rect35", (64, 48), "rect18", (80, 48), (8.0, 4.0, 3.0), 4),
]

# ---- the 30 cells: five output lenses x six source modes (clamped and wrapping equirectangular sources are two modes)
OUT_LENSES = ["rect18", "eqd_pi", "eqs", "stg", "eqr_part"]
SOURCES = [("rect18", (64, 48)), ("eqd_narrow", (64, 48)), ("eqr_part", (64, 32)), ("eqr_band", (64, 32)), ("eqs", (64, 48)), ("stg", (64, 48))]


# no rotation and a general one that turns the view round: the fisheye targets look along +z, the others along -z, so every cell
# sees the front of a folding source under one of the two and its back under the other
CELL_ROTATIONS = [None, (150.0, -15.0, 5.0)]


def cells():
    """(output lens, source lens, source size) of every cell; the output is 80 x 48."""
    return [(o, s, size) for o in OUT_LENSES for s, size in SOURCES]


# ---- the full frame: the BASELINE configs[3] geometry (an 18 mm rectilinear view into a full panorama, identity rotation matrix)
FULL_FRAME = dict(name="config3_4k_rect_pano", inp="rect18", in_size=(4096, 4096), out="eqr_full", out_size=(4096, 4096), deg=(0.0, 0.0, 0.0), n=1)
