"""The cases of the Lanczos-3 tests (include/lrp.h "Lanczos-3"), shared by tests/test_lanczos.py (CPU: the model against a
float64 restatement, the committed digests, the rule that every render discriminates), tests/test_gpu_lanczos.py (the HIP
output against the model bit for bit) and tests/golden/make_lanczos_golden.py."""
import math

import numpy as np

import cases
import coverage_cases as cc

LANCZOS3 = 3
POST = (2.0, 4.0)
SMALL = (2.0, 1.0, 0.5)  # pan, pitch, roll in degrees: a rotation that keeps a 1:1 mapping 1:1


def lens(lrp, name, w, h):
    if name == "rect_wide":  # a 161 degree view: minifies a fisheye in its middle, magnifies it towards its edges
        return lrp.LensInfo.rectilinear(3.0, 36.0, w, h)
    if name == "eqd_120":  # a 120 degree fisheye: more texels per radian than the 180 degree one
        return lrp.LensInfo.equidistant(2.0943951)
    return cc.lens(lrp, name, w, h)


def _case(name, inp, in_size, out, out_size, deg=None, C=4, ns=1, post=None, planted=False, exempt=False):
    return dict(name=name, inp=inp, in_size=in_size, out=out, out_size=out_size, deg=deg, C=C, ns=ns, post=post, planted=planted,
                exempt=exempt)


# ---- geometries: what the 6 x 6 footprints of a 32 x 8 tile look like in the source
GEOMETRY_CASES = [
    _case("pano_1to1", "eqr_full", (96, 48), "eqr_full", (96, 48), SMALL),            # 1:1, the footprints of a tile overlap almost entirely
    _case("tile_sees_pano", "eqr_full", (512, 256), "eqr_full", (32, 8)),             # one tile, 16 x minified: no two footprints overlap
    _case("fisheye_rect_mixed", "eqd_120", (192, 192), "rect_wide", (160, 96)),       # tiles differ
    _case("seam_pole_7x4", "eqr_full", (7, 4), "rect18", (33, 9), (180.0, 75.0, 0.0)),
    _case("seam_64x32_lon_pi", "eqr_full", (64, 32), "rect18", (40, 24), (180.0, 60.0, 0.0)),
    _case("source_3x2", "rect18", (3, 2), "rect35", (33, 9), (3.0, 1.0, 0.0), exempt=True),  # smaller than the footprint (6 texels: few values)
    _case("fisheye_out_nan_centre", "eqr_full", (64, 32), "eqd_pi", (33, 33)),        # the centre ray is NaN
    _case("planted_specials", "eqr_full", (48, 32), "rect18", (64, 40), cc.GENERAL, planted=True),
]

# ---- shapes and channels
SHAPE_CASES = (
    [_case(f"c{C}{'_post' if post else ''}", "eqd_pi", (21, 13), "rect18", (33, 9), cc.GENERAL, C=C, post=post)
     for C in (1, 3, 4, 5, 8, 11) for post in (None, POST)]
    + [_case(f"ns{ns}", "eqr_full", (21, 13), "eqd_pi", (33, 9), cc.GENERAL, ns=ns) for ns in (2, 3)]
    + [_case("ns2_c5_post", "eqr_part", (21, 13), "rect18", (33, 9), None, C=5, ns=2, post=POST),
       _case("out_1x1", "eqr_full", (21, 13), "rect18", (1, 1), cc.GENERAL, exempt=True),
       _case("out_31x8", "eqr_full", (21, 13), "rect18", (31, 8), cc.GENERAL),
       _case("out_64x16", "eqd_pi", (21, 13), "eqr_part", (64, 16), cc.GENERAL),
       _case("source_1x1", "rect18", (1, 1), "rect18", (33, 9), None, exempt=True),
       _case("source_2x2", "eqr_full", (2, 2), "rect18", (33, 9), cc.GENERAL, exempt=True)]
)

NAMED = GEOMETRY_CASES + SHAPE_CASES


def by_name(name):
    return next(c for c in NAMED if c["name"] == name)


def lenses(lrp, case):
    return lens(lrp, case["inp"], *case["in_size"]), lens(lrp, case["out"], *case["out_size"])


def rotation(lrp, case):
    return cases.rotation(lrp, case["deg"])


SPECIALS = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0x477FE000], dtype=np.uint32)  # -0, denormals, +-inf, NaN, 65504


def make_source(case, seed=1):
    """(H, W, C) float32: multiples of 1 / 2048 in [0, 1); planted: one texel each of SPECIALS, in every channel."""
    (w, h), C = case["in_size"], case["C"]
    a = cases.hash_noise(h, w, C, 0x1A2C0000 + seed, planted=False)
    if case["planted"]:
        rng = np.random.default_rng(seed)
        idx = rng.choice(w * h, size=SPECIALS.size, replace=False)
        a.reshape(w * h, C)[idx] = SPECIALS.view(np.float32)[:, None]
    return a


def model_render(lrp, lzm, case, src=None):
    lin, lout = lenses(lrp, case)
    src = make_source(case) if src is None else src
    (ow, oh) = case["out_size"]
    return lzm.reproject(lin, src, lout, ow, oh, case["ns"], rotation(lrp, case), case["post"])


def cell_cases():
    """The 30 cells of csrc/lrp_cells.h x {no rotation, a general one}: RGBA, 33 x 9 out of 21 x 13, num_samples 1."""
    out = []
    for o in cc.OUT_LENSES:
        for s, _ in cc.SOURCES:
            for rot, deg in (("norot", None), ("rot30", cc.GENERAL)):
                out.append(_case(f"cell_{o}_{s}_{rot}", s, (21, 13), o, (33, 9), deg))
    return out


def float64_weights(f):
    """sinc(d) sinc(d / 3) at the six tap distances of fraction(s) f, normalised, in float64: (..., 6)."""
    f = np.asarray(f, dtype=np.float64)[..., None]
    d = f - np.arange(-2, 4, dtype=np.float64)
    r = np.sinc(d) * np.sinc(d / 3.0)  # numpy's sinc is sin(pi x) / (pi x)
    return r / r.sum(axis=-1, keepdims=True)
