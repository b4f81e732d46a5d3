"""CPU: the coverage planes (include/lrp.h "coverage") without a GPU — the CPU model the GPU tests compare with
(tests/native/coverage_model.c): its render pinned to the stereographic model bit for bit on every cell, its coordinates to the
oracle's, its plane to the definition applied in numpy and to an independent float64 restatement of the lenses; the rule that
every case of tests/coverage_cases.py discriminates; and the argument errors of lrp_coverage_device, which are reported before
any device is touched."""
import ctypes
import json
import os

import numpy as np
import pytest

import cases
import coverage_cases as cc
import coverage_model as model
import stereographic_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLDING = (0, 1, 2, 3)  # lens types whose source side folds through x / -z


def geometry(lrp, case):
    (iw, ih), (ow, oh) = case["in_size"], case["out_size"]
    return cc.lens(lrp, case["inp"], iw, ih), iw, ih, cc.lens(lrp, case["out"], ow, oh), ow, oh, cases.rotation(lrp, case["deg"])


def wraps(lens):
    return lens.type == 4 and abs(float(np.float32(lens.params[3]) - np.float32(lens.params[2])) - 2 * np.pi) < np.float32(1e-5)


def definition(lens_in, iw, ih, sx, sy, vz):
    """include/lrp.h applied in numpy (binary32 comparisons; NaN compares false) to coordinates and rotated z."""
    with np.errstate(invalid="ignore"):
        front = (vz < np.float32(0.0)) if lens_in.type in FOLDING else np.ones(sx.shape, bool)
        in_x = (sx == sx) if wraps(lens_in) else ((sx >= np.float32(-0.5)) & (sx <= np.float32(iw) - np.float32(0.5)))
        in_y = (sy >= np.float32(-0.5)) & (sy <= np.float32(ih) - np.float32(0.5))
    return front & in_x & in_y


# ------------------------------------------------------------------ 1. the model's render is the stereographic model's
@pytest.mark.parametrize("out_name", cc.OUT_LENSES)
def test_render_equals_the_stereographic_model_on_every_cell(lrp, out_name):
    ow, oh = 23, 17
    rot = cases.rotation(lrp, cc.GENERAL)
    for k, (src_name, _) in enumerate(cc.SOURCES):
        iw, ih = 37, 29
        src = cases.hash_noise(ih, iw, 4, 3 + k)
        lin, lout = cc.lens(lrp, src_name, iw, ih), cc.lens(lrp, out_name, ow, oh)
        for interp, ns, r in ((0, 1, None), (1, 2, rot), (2, 3, rot)):
            cases.assert_same_bits(model.reproject(lin, src, lout, ow, oh, ns, interp, r),
                                   stereographic_model.reproject(lin, src, lout, ow, oh, ns, interp, r), f"{out_name}<-{src_name} interp {interp} ns {ns}")
    lin, lout = cc.lens(lrp, "eqd_pi", 32, 20), cc.lens(lrp, out_name, ow, oh)
    src3 = cases.hash_noise(20, 32, 3, 5)
    cases.assert_same_bits(model.reproject(lin, src3, lout, ow, oh, 1, 2, rot, post=(1.5, 4.0)),
                           stereographic_model.reproject(lin, src3, lout, ow, oh, 1, 2, rot, post=(1.5, 4.0)), "post")


# ------------------------------------------------------------------ 2. the reference's lenses: the oracle's coordinates
REFERENCE_CASES = [c for c in cc.CASES if not ({c["inp"], c["out"]} & {"eqs", "stg"})]


@pytest.mark.parametrize("case", REFERENCE_CASES, ids=[c["name"] for c in REFERENCE_CASES])
def test_n1_coordinates_equal_the_oracles_and_the_plane_is_the_definition(lrp, oracle, case):
    lin, iw, ih, lout, ow, oh, rot = geometry(lrp, case)
    plane, sxy, vz = model.coverage(lin, iw, ih, lout, ow, oh, 1, rot, detail=True)
    want = oracle.source_coords(lin, iw, ih, lout, ow, oh, rot)
    cases.assert_same_bits(sxy[:, :, 0, :], want, case["name"])  # NaNs included
    assert np.isnan(want).sum() == np.isnan(sxy).sum()
    covered = definition(lin, iw, ih, want[..., 0], want[..., 1], vz[:, :, 0])
    assert (plane == covered.astype(np.uint8)).all()


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_plane_is_the_definition_applied_to_the_models_sub_samples(lrp, case):
    lin, iw, ih, lout, ow, oh, rot = geometry(lrp, case)
    plane, sxy, vz = model.coverage(lin, iw, ih, lout, ow, oh, case["n"], rot, detail=True)
    covered = definition(lin, iw, ih, sxy[..., 0], sxy[..., 1], vz)
    assert (plane == covered.sum(axis=2)).all()
    assert (model.coverage(lin, iw, ih, lout, ow, oh, case["n"], rot) == plane).all()


# ------------------------------------------------------------------ 3. an independent float64 restatement
def ray64(lens, w, h, cx, cy):
    p = [float(np.float32(v)) for v in lens.params]
    sw, sh = float(lens.sensor_width), float(lens.sensor_height)
    with np.errstate(all="ignore"):
        if lens.type == 0:
            return cx / w * sw / p[0], cy / h * sh / p[0], -np.ones_like(cx)
        if lens.type == 4:
            lon = (cx / w + 0.5) * (p[3] - p[2]) + p[2]
            lat = (cy / h + 0.5) * (p[1] - p[0]) + p[0]
            return np.sin(lon), np.sin(lat), -np.cos(lon)
        r_mm = np.hypot(cx, cy) / w * sw
        theta = {1: lambda: r_mm * p[0] / sw, 2: lambda: 2.0 * np.arcsin(r_mm / (2.0 * p[0])), 3: lambda: 2.0 * np.arctan(r_mm / (2.0 * p[0]))}[lens.type]()
        s = np.sin(theta) / np.hypot(cx, cy)
        return s * cx, s * cy, np.cos(theta)


def source64(lens, w, h, x, y, z):
    p = [float(np.float32(v)) for v in lens.params]
    sw, sh = float(lens.sensor_width), float(lens.sensor_height)
    with np.errstate(all="ignore"):
        if lens.type == 4:
            theta = -np.arctan2(-x, -z)
            phi = np.arcsin(y / np.sqrt(x * x + y * y + z * z))
            return ((theta - p[2]) / (p[3] - p[2]) - 0.5) * w, ((phi - p[0]) / (p[1] - p[0]) - 0.5) * h
        u, v = x / -z, y / -z
        if lens.type == 0:
            return u * w / sw * p[0], v * h / sh * p[0]
        r = np.hypot(u, v)
        theta = np.arctan(r)
        r_mm = {1: lambda: theta * sw / p[0], 2: lambda: 2.0 * p[0] * np.sin(0.5 * theta), 3: lambda: 2.0 * p[0] * np.tan(0.5 * theta)}[lens.type]()
        return u / r * (r_mm / sw * w), v / r * (r_mm / sw * w)


def verdict64(lin, iw, ih, lout, ow, oh, n, rot):
    """(covered, doubtful) per sub-sample [oh][ow][n * n] in float64; doubtful: within 1e-3 px of a source border or |vz| < 1e-6."""
    y, x, ssx, ssy = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), np.arange(n, dtype=np.float64),
                                 np.arange(n, dtype=np.float64), indexing="ij")
    scx = (x + 0.5 - ow * 0.5 + (ssx + 1.0) / (n + 1.0) - 0.5).reshape(oh, ow, n * n)
    scy = (y + 0.5 - oh * 0.5 + (ssy + 1.0) / (n + 1.0) - 0.5).reshape(oh, ow, n * n)
    vx, vy, vz = ray64(lout, float(ow), float(oh), scx, scy)
    if rot is not None:
        R = np.asarray(rot, dtype=np.float64).reshape(3, 3)
        vx, vy, vz = (R[k, 0] * vx + R[k, 1] * vy + R[k, 2] * vz for k in range(3))
    px, py = source64(lin, float(iw), float(ih), vx, vy, vz)
    sx, sy = px - 0.5 + iw * 0.5, py - 0.5 + ih * 0.5
    folding = lin.type in FOLDING
    with np.errstate(invalid="ignore"):
        in_x = np.isfinite(sx) if wraps(lin) else ((sx >= -0.5) & (sx <= iw - 0.5))
        covered = (vz < 0.0 if folding else True) & in_x & (sy >= -0.5) & (sy <= ih - 0.5)
        near = (np.abs(sy + 0.5) < 1e-3) | (np.abs(sy - (ih - 0.5)) < 1e-3)
        if not wraps(lin):
            near |= (np.abs(sx + 0.5) < 1e-3) | (np.abs(sx - (iw - 0.5)) < 1e-3)
        if folding:
            near |= np.abs(vz) < 1e-6
    return covered, near


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_float64_restatement_gives_the_same_verdicts(lrp, case):
    lin, iw, ih, lout, ow, oh, rot = geometry(lrp, case)
    n = case["n"]
    _, sxy, vz = model.coverage(lin, iw, ih, lout, ow, oh, n, rot, detail=True)
    got = definition(lin, iw, ih, sxy[..., 0], sxy[..., 1], vz)
    want, doubtful = verdict64(lin, iw, ih, lout, ow, oh, n, rot)
    print(f"{case['name']}: {doubtful.mean():.4%} of the sub-samples left out, covered {want.mean():.3f}")
    assert doubtful.mean() <= 0.02, doubtful.mean()
    assert (got == want)[~doubtful].all(), np.argwhere((got != want) & ~doubtful)[:5]


# ------------------------------------------------------------------ 4. every case discriminates
@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_every_case_discriminates(lrp, case):
    lin, iw, ih, lout, ow, oh, rot = geometry(lrp, case)
    n = case["n"]
    plane = model.coverage(lin, iw, ih, lout, ow, oh, n, rot)
    none, full = (plane == 0).mean(), (plane == n * n).mean()
    partial = ((plane > 0) & (plane < n * n)).sum()
    print(f"{case['name']}: count 0 {none:.3f}, count n*n {full:.3f}, partial {partial} pixels")
    assert plane.max() <= n * n
    assert 0.05 <= none <= 0.95 and 0.05 <= full <= 0.95, (none, full)
    assert n == 1 or partial > 0


def test_the_front_case_passes_the_rectangle_test_everywhere(lrp):
    """eqd pi -> eqd 1.5 pi: every sub-sample with a ray lands inside the source rectangle, in front of the camera or behind it —
    vz alone decides, so a kernel without the vz test would call the whole frame covered."""
    case = next(c for c in cc.CASES if c["name"] == "eqd_eqd_front")
    lin, iw, ih, lout, ow, oh, rot = geometry(lrp, case)
    plane, sxy, vz = model.coverage(lin, iw, ih, lout, ow, oh, 1, rot, detail=True)
    inside = definition(cc.lens(lrp, "eqr_part", iw, ih), iw, ih, sxy[..., 0], sxy[..., 1], vz)[..., 0]  # (a lens without a front test)
    assert inside.all()
    assert 0.05 < (plane == 0).mean() < 0.95 and ((plane == 1) == (vz[..., 0] < 0)).all()


def test_full_frame_digest_is_the_models(lrp):
    """tests/golden/coverage_golden.json (what the GPU compares its 4096^2 plane with) is the model's: rendered here again."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_coverage_golden", os.path.join(ROOT, "tests", "golden", "make_coverage_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "coverage_golden.json")))
    assert golden["frame"] == gen.digest(cc.FULL_FRAME)
    assert 0.05 < golden["frame"]["count0"] / 4096 ** 2 < 0.95


# ------------------------------------------------------------------ 5. argument errors (no device is touched before them)
def _status(lrp, lin, lout, n=1, plane=True, mask=0, alpha=-1, channels=4, data=True):
    lib = lrp._native.load()
    cin = lrp.Image(lin, 8, 8, channels, None).to_c()
    cout = lrp.Image(lout, 8, 8, channels, None).to_c()
    cout.data = 0x1000 if data else None  # never dereferenced: every call here fails, in validation or at device -1
    return lib.lrp_coverage_device(ctypes.byref(cin), ctypes.byref(cout), n, None, 0x2000 if plane else None, mask, alpha, -1, None)


def test_argument_errors(lrp):
    S = lrp.Status
    rect, pano = lrp.LensInfo.rectilinear(18.0, 36.0, 8, 8), lrp.LensInfo.equirectangular()
    assert _status(lrp, rect, pano, plane=False) == S.BAD_ARG  # nothing requested
    assert _status(lrp, rect, pano, n=0) == S.BAD_ARG
    assert _status(lrp, rect, pano, n=16) == S.BAD_ARG
    assert _status(lrp, rect, pano, alpha=4) == S.BAD_ARG  # alpha_channel == channels
    assert _status(lrp, rect, pano, alpha=-2) == S.BAD_ARG
    assert _status(lrp, rect, pano, plane=False, mask=1, data=False) == S.NULL
    assert _status(lrp, rect, pano, plane=False, mask=1, channels=0) == S.CHANNELS
    assert "lrp_coverage_device" in lrp._native.SYMBOLS and "lrp_context_set_outside" in lrp._native.SYMBOLS
    assert lrp._native.load().lrp_abi_version() == 3
    # a good call gets as far as the device
    assert _status(lrp, rect, pano) == S.NO_DEVICE
    assert _status(lrp, rect, pano, n=15, plane=False, alpha=3) == S.NO_DEVICE


def test_extension_lenses_need_their_bit_like_reproject(lrp):
    S = lrp.Status
    good = lrp.LensInfo.rectilinear(18.0, 36.0, 8, 8)
    eqs, stg = lrp.LensInfo.equisolid(10.0, 36.0, 3.0, 8, 8), lrp.LensInfo.stereographic(10.0, 36.0, 8, 8)

    def reproject_status(lin, lout):
        a = np.zeros((8, 8, 4), dtype=np.float32)
        try:
            lrp.reproject(lrp.Image(lin, 8, 8, 4, a), lrp.Image(lout, 8, 8, 4, a.copy()), 1, 2)
        except lrp.LrpError as e:
            return e.status
        return 0

    assert lrp.lens_extensions() == 0
    try:
        for mask in (0, lrp.LENS_EXT_EQUISOLID, lrp.LENS_EXT_STEREOGRAPHIC):
            lrp.lens_extensions(mask)
            for lin, lout in ((good, eqs), (eqs, good), (good, stg), (stg, good), (eqs, stg), (stg, eqs)):
                want = reproject_status(lin, lout)
                if want in (S.OUTPUT_LENS, S.INPUT_LENS):
                    assert _status(lrp, lin, lout) == want, (mask, lin.type, lout.type)
                    assert _status(lrp, lin, lout, n=0, plane=False) == want  # (the lens errors come first)
                else:
                    assert _status(lrp, lin, lout, n=0) == S.BAD_ARG
    finally:
        lrp.lens_extensions(0)
    assert _status(lrp, good, stg) == S.OUTPUT_LENS
