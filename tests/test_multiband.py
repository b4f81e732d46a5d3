"""CPU: multi-band blending across a camera rig (include/lrp.h "multi-band blending across a camera rig").
The CPU model of tests/multiband_model.py against the numpy float32 restatement of tests/multiband_cases.py bit for bit, B == 0
against the per-label selection of one-camera renders, the winner rule, reconstruction, the discrimination of blending, both
error tables and the scratch size.  No device is touched."""
import ctypes
import math

import numpy as np
import pytest

import camera_cases as cam
import camera_gain_cases as gc
import camera_gain_model as gmodel
import camera_model as cmodel
import cases
import coverage_cases as cc
import multiband_cases as mb
import multiband_model as mmodel

F32 = np.float32


@pytest.fixture(autouse=True)
def extensions_on(lrp):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    try:
        yield
    finally:
        lrp.lens_extensions(prev)


def layers(cams, srcs, lout, ow, oh, interp, rots, gains=None):
    """G^i_0: the one-camera FIRST renders of the existing models."""
    out = []
    for i, (c, s) in enumerate(zip(cams, srcs)):
        rot = None if rots is None else [rots[i]]
        if gains is None:
            out.append(cmodel.compose([c], [s], lout, ow, oh, 1, interp, rot, 0)[0])
        else:
            out.append(gmodel.compose([c], [s], [gains[i]], lout, ow, oh, 1, interp, rot, 0)[0])
    return out


def winner_np(cams, lout, ow, oh, rots):
    """The winner rule restated on the camera model's per-pixel detail: (count, label)."""
    weights = []
    for i, c in enumerate(cams):
        _, sxy, _, covered = cmodel.detail(c, lout, ow, oh, 1, None if rots is None else rots[i])
        sx, sy, covered = sxy[:, :, 0, 0], sxy[:, :, 0, 1], covered[:, :, 0]
        w, h = F32(c["size"][0]), F32(c["size"][1])
        with np.errstate(all="ignore"):
            d = np.minimum(np.minimum(sx + F32(0.5), (w - F32(0.5)) - sx), np.minimum(sy + F32(0.5), (h - F32(0.5)) - sy))
        assert d.dtype == np.float32
        weights.append(np.where(covered, np.maximum(d, F32(2.0 ** -10)), F32(-1.0)))
    weights = np.stack(weights)
    count = (weights > 0).sum(axis=0).astype(np.uint8)
    label = np.where(count > 0, np.argmax(weights, axis=0), mb.NO_CAMERA).astype(np.uint8)  # (argmax: the first of equal maxima)
    return count, label


# ------------------------------------------------------------------ 1. the model is the definition
SIZES = [((1, 1), 3), ((2, 1), 3), ((5, 3), 3), ((33, 9), 3), ((33, 9), 1), (cam.OUT_SIZE, 5), (cam.OUT_SIZE, 8)]


@pytest.mark.parametrize("size,bands", SIZES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"B{v}")
@pytest.mark.parametrize("target", ["eqr_band", "cut", "eqr_part", "rect18"])
def test_model_is_the_numpy_restatement(lrp, target, size, bands):
    """A wrapping target (eqr_band, the rig across the +-180 degree seam), the same lens cut short of a full turn (clamps), and
    two targets the rig faces; levels of size 1 (1 x 1, 2 x 1, 5 x 3 with B = 3)."""
    ow, oh = size
    if target in ("eqr_band", "cut"):
        lout, cams, rots = mb.seam_rig(lrp, "eqr_band", size)
        if target == "cut":
            lout = mb.cut_lens(lrp)
    else:
        lout, cams, rots = cam.rig(lrp, target, size)
    wrap = target == "eqr_band"
    srcs = cam.sources(cams, 4)
    for interp, gains, post in ((2, None, None), (1, gc.GAINS, (2.0, 3.0))):
        got, count, label = mmodel.compose(cams, srcs, lout, ow, oh, interp, rots, bands, gains, post)
        want_count, want_label = winner_np(cams, lout, ow, oh, rots)
        assert (count == want_count).all() and (label == want_label).all()
        want = mb.blend_np(layers(cams, srcs, lout, ow, oh, interp, rots, gains), label, bands, wrap, post)
        cases.assert_same_bits(got, want, f"{target} {size} B {bands} interp {interp}")
    if size == cam.OUT_SIZE:
        assert len(set(np.unique(label)) - {mb.NO_CAMERA}) >= 2
        if target == "eqr_band":  # a label boundary crosses the seam, and the wrap changes bits
            assert (label[:, 0] != mb.NO_CAMERA).any() and (label[:, -1] != mb.NO_CAMERA).any()
            clamped = mb.blend_np(layers(cams, srcs, lout, ow, oh, interp, rots, gains), label, bands, False, post)
            assert (~cases.same_bits(clamped, want)).any()


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_zero_bands_select_the_winners_render(lrp, channels):
    """B == 0: +0.0f + G^winner_0, on frames with planted -0.0, denormal, inf and NaN texels."""
    lout, cams, rots = cam.rig(lrp, "eqr_part")
    ow, oh = cam.OUT_SIZE
    srcs = cam.sources(cams, channels, planted=True)
    seen_nan = seen_inf = False
    for interp in (0, 1, 2):
        got, count, label = mmodel.compose(cams, srcs, lout, ow, oh, interp, rots, 0)
        seen_nan, seen_inf = seen_nan or bool(np.isnan(got).any()), seen_inf or bool(np.isinf(got).any())
        g0 = layers(cams, srcs, lout, ow, oh, interp, rots)
        want = np.zeros_like(got)
        for i, g in enumerate(g0):
            with np.errstate(all="ignore"):
                want[label == i] = (F32(0.0) + g)[label == i]
        cases.assert_same_bits(got, want, f"C {channels} interp {interp}")
        assert not np.signbit(got[got == 0]).any()
    assert seen_nan and seen_inf and any(np.signbit(s[s == 0]).any() for s in srcs)


def test_winner_rule(lrp):
    ow, oh = cam.OUT_SIZE
    # ties go to the lowest index: a camera and its copy
    lout, cams, rots = cam.rig(lrp, "eqr_part")
    count, label = mmodel.labels([cams[0], cams[0], cams[1]], lout, ow, oh, [rots[0], rots[0], rots[1]])
    assert (label != 1).all() and (label == 0).any() and (label == 2).any() and (count[label == 0] >= 2).all()
    assert ((label == mb.NO_CAMERA) == (count == 0)).all() and (count == 0).any() and (count == 3).any()
    # eight cameras round the horizon, of which the copies 4 .. 7 of cameras 0 .. 3 win nowhere
    cams8, rots8 = cam.eight(lrp)
    cams8, rots8 = cams8[:4] + cams8[:4], rots8[:4] + rots8[:4]
    pano = cc.lens(lrp, "eqr_full", ow, oh)
    count, label = mmodel.labels(cams8, pano, ow, oh, rots8)
    want_count, want_label = winner_np(cams8, pano, ow, oh, rots8)
    assert (count == want_count).all() and (label == want_label).all()
    assert set(np.unique(label)) == {0, 1, 2, 3, mb.NO_CAMERA} and count.max() >= 4
    assert ((label == mb.NO_CAMERA) == (count == 0)).all()
    # and no rotations
    count, label = mmodel.labels(cams8[:3], lout, ow, oh, None)
    want_count, want_label = winner_np(cams8[:3], lout, ow, oh, None)
    assert (count == want_count).all() and (label == want_label).all()


def test_reconstruction(lrp):
    """One camera covers the whole target (the identity scene: every texel is its own pixel), so M = 1 everywhere and the result
    is that camera's render up to rounding: the largest error per B, in ulps of the render's largest value (the rounding of
    (G - E) + E is on the scale of the blur E, not of the pixel), against twice what was measured on the model."""
    lout = cam.identity_lens(lrp)
    # (the noise itself is dyadic and within a factor of two of its blur: (G - E) + E would be exact.  Squared and scaled it spans
    # 0 .. 3.1 with many values near 0.)
    srcs = [(s - F32(0.25)) * (s - F32(0.25)) * F32(3.1) for s in cam.sources([cam.IDENTITY], 4)]
    render = cmodel.compose([cam.IDENTITY], srcs, lout, 64, 32, 1, 1, None, 0)[0]
    for bands, measured in mb.RECONSTRUCTION_ULPS_MEASURED.items():
        got, count, label = mmodel.compose([cam.IDENTITY], srcs, lout, 64, 32, 1, None, bands)
        assert (count == 1).all() and (label == 0).all()
        worst = float(mb.ulps_of_scale(got, render).max())
        print(f"reconstruction B {bands}: max error {worst:.2f} ulps (measured {measured}, bound {2 * measured})")
        assert worst <= 2 * measured


def test_blending_discriminates(lrp):
    """The recovery scene of the exposure-matching tests, no gains: the step across the seams under B = 4 is below the one under
    B = 0 by at least half the improvement measured on the model; with equal exposures B = 4 stays within twice the measured
    difference of FEATHER."""
    ow, oh = cam.OUT_SIZE
    lout, cams, rots, srcs = gc.recovery_scene(lrp)
    step = {}
    for bands in (0, 4):
        img, count, label = mmodel.compose(cams, srcs, lout, ow, oh, 1, rots, bands)
        step[bands] = mb.seam_step(img, label)
    measured = mb.SEAM_STEP_MEASURED
    print(f"seam step: B 0 {step[0]:.5f}, B 4 {step[4]:.5f} (measured {measured[0]}, {measured[4]}): improvement {step[0] - step[4]:.5f}")
    assert measured[0] > measured[4] and step[0] - step[4] >= 0.5 * (measured[0] - measured[4])
    lout, cams, rots, srcs = mb.equal_exposure_scene(lrp)
    img, count, label = mmodel.compose(cams, srcs, lout, ow, oh, 1, rots, 4)
    feather = cmodel.compose(cams, srcs, lout, ow, oh, 1, 1, rots, 2)[0]
    diff = float(np.abs(img[..., :3].astype(np.float64) - feather[..., :3])[count > 0].max())
    print(f"equal exposures: max |B 4 - FEATHER| {diff:.5f} (measured {mb.FEATHER_DIFFERENCE_MEASURED})")
    assert diff <= 2 * mb.FEATHER_DIFFERENCE_MEASURED


# ------------------------------------------------------------------ the error tables, in order, without a device
def _good(lrp, model=0):
    c = cam.product(lrp, cam.camera(model, (8, 8), 6.0, 6.0, 3.5, 3.5, (0.01, 0.001, 0.001, 0.001, 0.001), limit=1.0)).to_c()
    c.data = 0x1000  # never dereferenced: every call here fails, in validation or at device -1
    return c


def _with(c, **fields):
    d = type(c)()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(c), ctypes.sizeof(c))
    for name, value in fields.items():
        setattr(d, name, value)
    return d


def _call(lrp, cams, gains=None, interp=2, bands=3, scratch=0x100000, scratch_bytes=None, null_cams=False, null_out=False, lout=None,
          out_channels=4, out_size=(8, 8), out_data=0x2000):
    lib = lrp._native.load()
    k = len(cams)
    arr = (lrp._native.LrpCamera * max(k, 1))(*cams)
    cout = lrp.Image(lout or lrp.LensInfo.equirectangular(), out_size[0], out_size[1], out_channels, None).to_c()
    cout.data = out_data
    g = None if gains is None else np.asarray(gains, dtype=np.float32)
    if scratch_bytes is None:
        scratch_bytes = 1 << 40
    st = lib.lrp_compose_cameras_multiband_device(None if null_cams else arr, k, None, None if g is None else g.ctypes.data,
                                                  None if null_out else ctypes.byref(cout), interp, bands, None, None, None, scratch, scratch_bytes,
                                                  -1, None)
    return st, lib.lrp_last_error().decode()


def test_multiband_argument_errors(lrp):
    S, L = lrp.Status, lrp.LensInfo
    good, fish = _good(lrp), _good(lrp, 1)
    nan = math.nan
    bad_cam = _with(good, model=5)
    need = lrp.multiband_scratch_bytes(8, 8, 4, 3)
    # good calls get as far as the device: every band count, every sampler, gains or none, the exact scratch size
    for bands in range(9):
        assert _call(lrp, [good, fish, good], bands=bands, interp=bands % 3)[0] == S.NO_DEVICE
    assert _call(lrp, [good] * 8, gains=[0.0] * 8, scratch_bytes=need)[0] == S.NO_DEVICE
    for channels in (1, 2, 3, 4):
        assert _call(lrp, [good], out_channels=channels)[0] == S.NO_DEVICE
    # 1. the checks of the gained compose, in their order: n_in; NULL; the output side; the interpolation; the cameras; the gains
    for k in (0, 9):
        st, text = _call(lrp, [good] * k, null_out=True, interp=7, bands=9, scratch=None)
        assert st == S.BAD_ARG and "n_in" in text
    assert _call(lrp, [good], null_cams=True, interp=7, bands=9)[0] == S.NULL and _call(lrp, [good], null_out=True, bands=9)[0] == S.NULL
    lrp.lens_extensions(0)
    assert _call(lrp, [bad_cam], lout=L.stereographic(10.0, 36.0, 8, 8), interp=7, out_channels=0)[0] == S.OUTPUT_LENS
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    assert _call(lrp, [bad_cam], interp=7, out_channels=0, out_size=(0, 8))[0] == S.CHANNELS
    assert _call(lrp, [bad_cam], interp=7, out_size=(0, 8), out_data=None, out_channels=5)[0] == S.BAD_DIMS
    assert _call(lrp, [bad_cam], interp=7, out_data=None, out_channels=5)[0] == S.NULL
    assert _call(lrp, [bad_cam], gains=[nan], interp=7, out_channels=5)[0] == S.INTERPOLATION
    assert _call(lrp, [bad_cam], gains=[nan], interp=3, out_channels=5)[0] == S.INTERPOLATION  # (Lanczos-3 is out of scope)
    st, text = _call(lrp, [good, bad_cam], gains=[nan, nan], out_channels=5, bands=9)
    assert st == S.BAD_ARG and "camera 1" in text and "model" in text
    st, text = _call(lrp, [good, _with(good, data=None)], gains=[nan, nan], out_channels=5)
    assert st == S.NULL and "camera 1" in text
    for bad in (nan, math.inf, -1.0):
        st, text = _call(lrp, [good, fish, good], gains=[1.0, 1.0, bad], out_channels=5, bands=9, scratch=None)
        assert st == S.BAD_ARG and "camera 2" in text and "gain" in text
    # 2. more than 4 channels, before the bands
    st, text = _call(lrp, [good], out_channels=5, bands=9, scratch=None)
    assert st == S.CHANNELS
    # 3. the bands, before the scratch
    for bands in (-1, 9):
        st, text = _call(lrp, [good], bands=bands, scratch=None)
        assert st == S.BAD_ARG and "num_bands" in text
    # 4. scratch NULL, before its size
    st, text = _call(lrp, [good], scratch=None, scratch_bytes=0)
    assert st == S.NULL and "scratch" in text
    # 5. alignment and size: the text states both sizes
    for scratch, size in ((0x100000 + 128, need), (0x100000, need - 1), (0x100000, 0)):
        st, text = _call(lrp, [good], scratch=scratch, scratch_bytes=size)
        assert st == S.BAD_ARG and str(size) in text and str(need) in text, text
    # 6. a target taller than a launch grid of 8-row tiles, last
    assert _call(lrp, [good], out_size=(1, 8 * 65535), out_channels=1)[0] == S.NO_DEVICE
    st, text = _call(lrp, [good], out_size=(1, 8 * 65535 + 1), out_channels=1)
    assert st == S.BAD_DIMS and "height" in text
    assert _call(lrp, [good], out_size=(1, 8 * 65535 + 1), out_channels=1, scratch_bytes=0)[0] == S.BAD_ARG
    for name in ("lrp_multiband_scratch_bytes", "lrp_compose_cameras_multiband_device"):
        assert name in lrp._native.SYMBOLS
    assert lrp._native.load().lrp_abi_version() == 3 and lrp.MULTIBAND_MAX_BANDS == 8 and lrp.MULTIBAND_NO_CAMERA == 255


def test_scratch_bytes(lrp):
    S = lrp.Status
    lib = lrp._native.load()
    for w, h in ((1, 1), (2, 1), (5, 3), (33, 9), (80, 48), (4096, 2048), (1, 7000)):
        for channels in (1, 2, 3, 4):
            for bands in range(9):
                got = lrp.multiband_scratch_bytes(w, h, channels, bands)
                assert got == mb.scratch_bytes(w, h, channels, bands) and got % 256 == 0, (w, h, channels, bands)
    assert lrp.multiband_scratch_bytes(4096, 2048, 4, 5) > 2 * 4096 * 2048 * 16
    out = ctypes.c_size_t(77)
    call = lambda w, h, c, b, p=ctypes.byref(out): lib.lrp_multiband_scratch_bytes(w, h, c, b, p)
    assert call(0, 0, 0, 9, None) == S.NULL
    for w, h in ((0, 8), (8, 0), (-1, 8)):
        assert call(w, h, 0, 9) == S.BAD_DIMS
    for channels in (0, 5, -1):
        assert call(8, 8, channels, 9) == S.CHANNELS
    for bands in (-1, 9):
        assert call(8, 8, 4, bands) == S.BAD_ARG
    assert out.value == 77 and call(8, 8, 4, 8) == S.OK and out.value == mb.scratch_bytes(8, 8, 4, 8)
