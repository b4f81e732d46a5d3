"""CPU: compose with calibrated cameras (include/lrp.h "compose, calibrated cameras") without a GPU — the CPU model the GPU
tests compare with (tests/native/camera_model.c) against a float64 evaluation of the two polynomials written here in numpy; the
conventions (axes, pixel origin, focal lengths in pixels) pinned to the existing rectilinear and equidistant lenses of the
coverage model; lrp_camera_limit; the ghost that `limit` removes; the scenes of tests/camera_cases.py discriminate; and the
error table of lrp_compose_cameras_device, each error before any device call."""
import ctypes
import math

import numpy as np
import pytest

import camera_cases as cam
import camera_model as cmodel
import cases
import coverage_cases as cc
import coverage_model as model

# The bound tests/test_stereographic.py uses for coordinates at these sizes (sources of about 64 x 48, fx 30 .. 60): binary32
# against float64, in pixels.
COORD_TOL_PX = 1e-3


@pytest.fixture(autouse=True)
def extensions_on(lrp):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    try:
        yield
    finally:
        lrp.lens_extensions(prev)


# ------------------------------------------------------------------ 1. the model against float64
@pytest.mark.parametrize("index", [0, 1, 2], ids=["brown_wide", "fisheye", "brown_mild"])
def test_model_against_float64(lrp, index):
    """sx, sy of the model against numpy float64 on a grid of rays, every kind of coefficient non-zero.  BROWN: rays up to 50
    degrees off axis in x and in y (the imaged ones are compared); FISHEYE: up to 100 degrees, beyond the hemisphere."""
    c = cam.resolve(lrp, cam.RIG[index])
    assert all(k != 0.0 for k in c["k"])
    rays = cam.ray_grid(math.radians(100.0 if c["model"] == cam.FISHEYE else 50.0))
    sxy, imaged = cmodel.project(c, rays)
    want = cam.project64(c, rays)
    assert imaged.mean() > 0.5
    err = np.abs(sxy[imaged].astype(np.float64) - want[imaged]).max()
    print(f"camera {index}: {int(imaged.sum())} rays, largest |model - float64| = {err:.3g} px")
    assert err <= COORD_TOL_PX
    if c["model"] == cam.FISHEYE:
        assert (rays[imaged][:, 2] > 0).any(), "no ray behind the camera in the fisheye grid"


def _near_frame(sxy, w, h):
    """The sub-samples whose coordinates lie in the frame or within half a frame of it (coordinates of rays far outside grow
    without bound, and an absolute bound says nothing there)."""
    with np.errstate(invalid="ignore"):
        return (sxy[..., 0] > -0.5 * w) & (sxy[..., 0] < 1.5 * w) & (sxy[..., 1] > -0.5 * h) & (sxy[..., 1] < 1.5 * h)


def test_brown_without_distortion_is_the_rectilinear_lens(lrp):
    """k = 0, fx = in_w / sensor_width * focal, fy = in_h / sensor_height * focal, cx = in_w / 2 - 0.5, cy = in_h / 2 - 0.5: the
    coverage model's rectilinear sx, sy — axes, the pixel origin and the units are the library's."""
    w, h = 64, 48
    lens = cc.lens(lrp, "rect18", w, h)
    pano = cc.lens(lrp, "eqr_full", 96, 48)
    rot = cases.rotation(lrp, cc.GENERAL)
    c = cam.camera(cam.BROWN, (w, h), w / lens.sensor_width * 18.0, h / lens.sensor_height * 18.0, w / 2 - 0.5, h / 2 - 0.5, (0.0,) * 5, cam.INF)
    for n in (1, 2):
        plane, want, vz = model.coverage(lens, w, h, pano, 96, 48, n, rot, detail=True)
        _, sxy, imaged, covered = cmodel.detail(c, pano, 96, 48, n, rot)
        assert (imaged == (vz < 0)).all()
        near = imaged & _near_frame(want, w, h)
        assert near.mean() > 0.1
        err = np.abs(sxy[near].astype(np.float64) - want[near]).max()
        print(f"n {n}: {int(near.sum())} sub-samples, largest difference {err:.3g} px")
        assert err <= COORD_TOL_PX
        # and the coverage: equal wherever no coordinate lies within the bound of the frame's edge
        edge = np.minimum(np.abs(want + 0.5), np.abs(want - (np.array([w, h], dtype=np.float32) - 0.5))).min(axis=-1) <= COORD_TOL_PX
        assert (covered.sum(axis=2) == plane)[~edge.any(axis=2)].all()


def test_fisheye_without_distortion_is_the_equidistant_lens(lrp):
    """k = 0, fx = fy = in_w / fov and the same centre: the coverage model's equidistant sx, sy on the front hemisphere."""
    w, h = 64, 48
    lens = cc.lens(lrp, "eqd_pi", w, h)
    pano = cc.lens(lrp, "eqr_full", 96, 48)
    rot = cases.rotation(lrp, cc.GENERAL)
    c = cam.camera(cam.FISHEYE, (w, h), w / math.pi, w / math.pi, w / 2 - 0.5, h / 2 - 0.5, (0.0,) * 4, math.pi)
    for n in (1, 2):
        _, want, vz = model.coverage(lens, w, h, pano, 96, 48, n, rot, detail=True)
        ray, sxy, imaged, _ = cmodel.detail(c, pano, 96, 48, n, rot)
        assert (ray[..., 2] == vz).all() and imaged.all()
        front = vz < 0
        assert 0.3 < front.mean() < 0.7
        err = np.abs(sxy[front].astype(np.float64) - want[front]).max()
        print(f"n {n}: {int(front.sum())} sub-samples, largest difference {err:.3g} px")
        assert err <= COORD_TOL_PX
        # behind the camera the two part: the equidistant lens folds through x / -z, the camera does not
        assert np.abs(sxy[~front] - want[~front]).max() > 1.0


# ------------------------------------------------------------------ 2. lrp_camera_limit
def test_camera_limit(lrp):
    brown = lambda k: cam.product(lrp, cam.camera(cam.BROWN, (64, 48), 50.0, 50.0, 31.5, 23.5, k))
    fish = lambda k: cam.product(lrp, cam.camera(cam.FISHEYE, (64, 48), 50.0, 50.0, 31.5, 23.5, k))
    # BROWN, k1 = -0.3 alone: d/dr (r - 0.3 r^3) = 0 at r2 = 1 / 0.9
    t = 1.0 / 0.9
    v = lrp.camera_limit(brown((-0.3, 0.0, 0.0, 0.0, 0.0)))
    print(f"BROWN k1 = -0.3: limit {v!r}, turning point {t!r}")
    assert 0.99 * t <= v <= t
    assert brown((-0.3, 0.0, 0.0, 0.0, 0.0)).limit == v  # limit=None asks the helper
    # the tangential terms do not enter
    assert lrp.camera_limit(brown((-0.3, 0.0, 0.01, -0.02, 0.0))) == v
    # FISHEYE, k1 = -0.1 alone: d/dtheta (theta - 0.1 theta^3) = 0 at theta = sqrt(1 / 0.3)
    t = math.sqrt(1.0 / 0.3)
    v = lrp.camera_limit(fish((-0.1, 0.0, 0.0, 0.0)))
    print(f"FISHEYE k1 = -0.1: limit {v!r}, turning point {t!r}")
    assert 0.99 * t <= v <= t
    # a small turning point keeps the relative guarantee: k1 = -100 turns at r2 = 1 / 300
    t = 1.0 / 300.0
    v = lrp.camera_limit(brown((-100.0, 0.0, 0.0, 0.0, 0.0)))
    assert 0.99 * t <= v <= t
    # all-zero coefficients, and polynomials that increase all the way
    assert lrp.camera_limit(brown((0.0,) * 5)) == math.inf
    assert lrp.camera_limit(fish((0.0,) * 4)) == float(np.float32(math.pi))
    assert lrp.camera_limit(brown((0.1, 0.01, 0.3, 0.3, 0.001))) == math.inf
    assert lrp.camera_limit(fish(cam.FISHEYE_K)) == float(np.float32(math.pi))
    # the wide lens of the cases: near r = 1.86 (numpy: the root of 1 + 3 k1 r^2 + 5 k2 r^4 + 7 k3 r^6)
    k1, k2, _, _, k3 = (float(np.float32(k)) for k in cam.BROWN_WIDE)  # (the coefficients the library sees: binary32)
    roots = np.roots([7 * k3, 0, 5 * k2, 0, 3 * k1, 0, 1.0])
    t = min(r.real for r in roots if abs(r.imag) < 1e-12 and r.real > 0) ** 2
    v = lrp.camera_limit(brown(cam.BROWN_WIDE))
    assert abs(math.sqrt(t) - 1.86) < 0.01 and 0.99 * t <= v <= t
    # errors
    lib, S = lrp._native.load(), lrp.Status
    c, out = brown((0.0,) * 5).to_c(), ctypes.c_float()
    assert lib.lrp_camera_limit(None, ctypes.byref(out)) == S.NULL and lib.lrp_camera_limit(ctypes.byref(c), None) == S.NULL
    c.model = 2
    assert lib.lrp_camera_limit(ctypes.byref(c), ctypes.byref(out)) == S.BAD_ARG
    c.model, c.k[4] = 1, math.nan  # FISHEYE ignores k[4]
    assert lib.lrp_camera_limit(ctypes.byref(c), ctypes.byref(out)) == S.OK
    c.k[3] = math.inf
    assert lib.lrp_camera_limit(ctypes.byref(c), ctypes.byref(out)) == S.BAD_ARG and "k[3]" in lib.lrp_last_error().decode()


# ------------------------------------------------------------------ 3. the ghost that `limit` removes
def test_limit_removes_the_ghost(lrp):
    """The wide lens's polynomial turns near r = 1.86 and comes back: rays far outside the field of view land inside the frame
    again.  With the helper's limit the model leaves every ray with r2 > limit uncovered; with limit = +inf it covers some."""
    pano = cc.lens(lrp, "eqr_full", 96, 48)
    wide = cam.camera(cam.BROWN, (64, 48), 20.0, 20.0, 31.5, 23.5, cam.BROWN_WIDE)
    limited = cam.resolve(lrp, wide)
    assert 1.8 ** 2 < limited["limit"] < 1.9 ** 2
    for n in (1, 2):
        ray, _, imaged, covered = cmodel.detail(limited, pano, 96, 48, n)
        with np.errstate(all="ignore"):
            r2 = (ray[..., 0] / -ray[..., 2]) ** 2 + (ray[..., 1] / -ray[..., 2]) ** 2
        beyond = (ray[..., 2] < 0) & (r2 > np.float32(limited["limit"]) * np.float32(1.001))  # (clear of the rounding of r2 itself)
        assert beyond.mean() > 0.05 and not covered[beyond].any() and not imaged[beyond].any() and covered.any()
        _, _, _, ghost = cmodel.detail(dict(wide, limit=cam.INF), pano, 96, 48, n)
        print(f"n {n}: {int(ghost[beyond].sum())} of {int(beyond.sum())} sub-samples beyond the limit are ghosts without it")
        assert ghost[beyond].any() and (ghost[~beyond] == covered[~beyond]).mean() > 0.999
    # the image: uncovered pixels are +0.0, and the ghost pixels of the unlimited camera are not
    src = cam.sources([wide], channels=3)
    got, count, m = cmodel.compose([limited], src, pano, 96, 48, 2, 1)
    unl, _, m_unl = cmodel.compose([dict(wide, limit=cam.INF)], src, pano, 96, 48, 2, 1)
    assert ((got.view(np.uint32) == 0).all(axis=2) == (m == 0)).all() and (m_unl >= m).all() and (m_unl > m).any() and (count == (m > 0)).all()
    assert (unl[(m == 0) & (m_unl > 0)] != 0).all()


# ------------------------------------------------------------------ 4. the scenes of the GPU test discriminate
@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_rig_scenes_discriminate(lrp, out_name):
    lout, cams, rots = cam.rig(lrp, out_name)
    assert [c["model"] for c in cams] == [cam.BROWN, cam.FISHEYE, cam.BROWN]
    ow, oh = cam.OUT_SIZE
    srcs = cam.sources(cams, channels=1)
    for n in (2, 3):
        _, count, m = cmodel.compose(cams, srcs, lout, ow, oh, n, 0, rots, 1)
        print(f"{out_name} n {n}: m == 0 {int((m == 0).sum())}, partial {int(((m > 0) & (m < n * n)).sum())}, full {int((m == n * n).sum())}, "
              f"count >= 2 {int((count >= 2).sum())}, count == 3 {int((count == 3).sum())}")
        assert cam.discriminates(count, m, n)
        # the planes are the definition per sub-sample
        cov = np.stack([cmodel.detail(c, lout, ow, oh, n, r)[3] for c, r in zip(cams, rots)])
        assert (cov.any(axis=3).sum(axis=0) == count).all() and ((cov.sum(axis=0) > 0).sum(axis=2) == m).all()


def test_modes_differ_where_cameras_overlap(lrp):
    lout, cams, rots = cam.rig(lrp, "eqr_part")
    srcs = cam.sources(cams)
    first, count, _ = cmodel.compose(cams, srcs, lout, 80, 48, 2, 1, rots, 0)
    mean, _, _ = cmodel.compose(cams, srcs, lout, 80, 48, 2, 1, rots, 1)
    feather, _, _ = cmodel.compose(cams, srcs, lout, 80, 48, 2, 1, rots, 2)
    for a, b in ((first, mean), (mean, feather), (first, feather)):
        assert (~cases.same_bits(a, b)).any(axis=2)[count >= 2].mean() > 0.5
    cases.assert_same_bits(mean[count == 1], first[count == 1], "MEAN of one camera")


def test_fisheye_200_sees_behind_itself(lrp):
    pano = cc.lens(lrp, "eqr_full", 96, 48)
    ray, _, imaged, covered = cmodel.detail(cam.FISHEYE_200, pano, 96, 48, 1)
    assert (covered & (ray[..., 2] >= 0)).any() and (covered & (ray[..., 2] < 0)).any() and not covered.all()


def test_identity(lrp):
    """A 64 x 32 rectilinear target (focal 16, sensor 32 x 16) and an undistorted camera of the same pinhole: sx == x and sy == y
    exactly, so every sampler returns the source bit for bit (Catmull-Rom at t = 0 is b + 0 * (...) = b for finite texels)."""
    lens = cam.identity_lens(lrp)
    _, sxy, imaged, covered = cmodel.detail(cam.IDENTITY, lens, 64, 32, 1)
    ys, xs = np.mgrid[0:32, 0:64]
    assert (sxy[:, :, 0, 0] == xs).all() and (sxy[:, :, 0, 1] == ys).all() and covered.all()
    src = cam.sources([cam.IDENTITY])
    for interp in (0, 1, 2):
        got, count, m = cmodel.compose([cam.IDENTITY], src, lens, 64, 32, 1, interp)
        cases.assert_same_bits(got, src[0], f"interp {interp}")
        assert (count == 1).all() and (m == 1).all()


# ------------------------------------------------------------------ 5. argument errors (no device is touched before them)
def _call(lrp, cams, lout=None, n=2, mode=0, interp=2, out_channels=4, out_size=(8, 8), out_data=0x2000, null_cams=False, null_out=False):
    lib = lrp._native.load()
    k = len(cams)
    arr = (lrp._native.LrpCamera * max(k, 1))(*cams)
    cout = lrp.Image(lout or lrp.LensInfo.equirectangular(), out_size[0], out_size[1], out_channels, None).to_c()
    cout.data = out_data
    st = lib.lrp_compose_cameras_device(None if null_cams else arr, k, None, None if null_out else ctypes.byref(cout), n, interp, mode, None,
                                        None, None, -1, None)
    return st, lib.lrp_last_error().decode()


def _good(lrp, model=0):
    c = cam.product(lrp, cam.camera(model, (8, 8), 6.0, 6.0, 3.5, 3.5, (0.01, 0.001, 0.001, 0.001, 0.001), limit=1.0)).to_c()
    c.data = 0x1000  # never dereferenced: every call here fails, in validation or at device -1
    return c


def _with(c, **fields):
    d = type(c)()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(c), ctypes.sizeof(c))
    for name, value in fields.items():
        if name.startswith("k"):
            d.k[int(name[1:])] = value
        else:
            setattr(d, name, value)
    return d


def test_argument_errors(lrp):
    S, L = lrp.Status, lrp.LensInfo
    good, fish = _good(lrp), _good(lrp, 1)
    nan, inf = math.nan, math.inf
    # good calls get as far as the device: both models, mixed, every n and mode
    for n in range(1, 16):
        assert _call(lrp, [good, fish, good], n=n, mode=n % 3, interp=n % 3)[0] == S.NO_DEVICE
    assert _call(lrp, [_with(good, limit=inf), _with(fish, k4=nan, limit=0.0)])[0] == S.NO_DEVICE  # +inf, 0 and an unused k are fine
    # 1. n_in, mode — before anything else
    for k in (0, 9):
        st, text = _call(lrp, [good] * k, n=16, interp=7, null_out=True)
        assert st == S.BAD_ARG and "n_in" in text
    st, text = _call(lrp, [good], mode=3, null_cams=True)
    assert st == S.BAD_ARG and "mode" in text
    # 2. NULL
    assert _call(lrp, [good], null_cams=True, interp=7)[0] == S.NULL and _call(lrp, [good], null_out=True, interp=7)[0] == S.NULL
    # 3. the output side, before the interpolation and the cameras
    bad_cam = _with(good, model=5)
    lrp.lens_extensions(0)
    assert _call(lrp, [bad_cam], lout=L.stereographic(10.0, 36.0, 8, 8), interp=7, out_channels=0)[0] == S.OUTPUT_LENS
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    assert _call(lrp, [good], lout=L.stereographic(10.0, 36.0, 8, 8))[0] == S.NO_DEVICE
    assert _call(lrp, [bad_cam], interp=7, out_channels=0, out_size=(0, 8))[0] == S.CHANNELS
    assert _call(lrp, [bad_cam], interp=7, out_size=(0, 8), out_data=None)[0] == S.BAD_DIMS
    assert _call(lrp, [bad_cam], interp=7, out_size=(1 << 15, 1 << 15), out_data=None)[0] == S.BAD_DIMS  # 2^32 floats
    assert _call(lrp, [bad_cam], interp=7, out_data=None)[0] == S.NULL
    # 4. interpolation, before the cameras; Lanczos-3 is not taken even with its extension on
    assert _call(lrp, [bad_cam], interp=7, n=0)[0] == S.INTERPOLATION and _call(lrp, [bad_cam], interp=-1)[0] == S.INTERPOLATION
    prev = lrp.sampler_extensions(lrp.SAMPLER_EXT_LANCZOS3)
    try:
        assert _call(lrp, [good], interp=3)[0] == S.INTERPOLATION
    finally:
        lrp.sampler_extensions(prev)
    # 5. per camera, ascending, and within a camera in the order model, size, data, values
    st, text = _call(lrp, [good, bad_cam, _with(good, width=0)], n=0)
    assert st == S.BAD_ARG and "camera 1" in text and "model" in text
    st, text = _call(lrp, [good, _with(good, width=0, data=None), bad_cam], n=0)
    assert st == S.BAD_DIMS and "camera 1" in text
    assert _call(lrp, [_with(good, height=-3, data=None)])[0] == S.BAD_DIMS
    st, text = _call(lrp, [_with(fish, width=1 << 15, height=1 << 15, data=None, fx=nan)])  # 2^30 texels of 4 channels
    assert st == S.BAD_DIMS and "camera 0" in text
    assert _call(lrp, [_with(fish, width=1 << 15, height=1 << 14)])[0] == S.NO_DEVICE  # 2^31 floats: the largest frame
    st, text = _call(lrp, [good, good, _with(good, data=None, fx=nan)], n=0)
    assert st == S.NULL and "camera 2" in text
    for field in ("fx", "fy", "cx", "cy"):
        for bad in (nan, inf, -inf):
            st, text = _call(lrp, [good, _with(fish, **{field: bad})], n=0)
            assert st == S.BAD_ARG and "camera 1" in text and field in text, (field, bad, text)
    for j in range(5):
        st, text = _call(lrp, [_with(good, **{f"k{j}": nan}), good], n=0)
        assert st == S.BAD_ARG and "camera 0" in text and f"k[{j}]" in text
    for j in range(4):
        st, text = _call(lrp, [good, good, good, _with(fish, **{f"k{j}": -inf})])
        assert st == S.BAD_ARG and "camera 3" in text and f"k[{j}]" in text
    for field in ("fx", "fy"):
        for zero in (0.0, -0.0):
            st, text = _call(lrp, [_with(good, **{field: zero})])
            assert st == S.BAD_ARG and "camera 0" in text and field in text
    assert _call(lrp, [_with(good, fx=-6.0, fy=-6.0, cx=0.0, cy=-100.0)])[0] == S.NO_DEVICE  # negative focal lengths mirror; allowed
    for bad in (nan, -1.0, -inf):
        st, text = _call(lrp, [good, _with(fish, limit=bad)])
        assert st == S.BAD_ARG and "camera 1" in text and "limit" in text
    # 6. num_samples last
    for n in (0, -1, 16):
        st, text = _call(lrp, [good, fish], n=n)
        assert st == S.BAD_ARG and "num_samples" in text
    assert "lrp_compose_cameras_device" in lrp._native.SYMBOLS and "lrp_camera_limit" in lrp._native.SYMBOLS
    assert lrp._native.load().lrp_abi_version() == 3


def test_tensors_are_checked_in_python(lrp):
    import torch

    pano = lrp.LensInfo.equirectangular()
    host = np.zeros((8, 8, 4), dtype=np.float32)
    mk = lambda data: lrp.Camera.brown(8, 8, data, 6.0, 6.0, 3.5, 3.5)
    assert mk(None).limit == math.inf and lrp.Camera.fisheye(8, 8, None, 6.0, 6.0, 3.5, 3.5).limit == float(np.float32(math.pi))
    assert lrp.Camera.brown(8, 8, None, 6.0, 6.0, 3.5, 3.5, limit=2.5).limit == 2.5 and mk(None).model == lrp.CameraModel.BROWN
    out = lrp.Image(pano, 16, 8, 4, None)
    for data, out_data in ((host, np.zeros((8, 16, 4), dtype=np.float32)), (torch.from_numpy(host), torch.zeros((8, 16, 4))), (None, None)):
        with pytest.raises(ValueError, match="device tensors only"):
            lrp.compose_cameras([mk(data)], lrp.Image(pano, 16, 8, 4, out_data), 2, 2)
    for bad in (torch.zeros((8, 16), dtype=torch.float32), torch.zeros((8, 15), dtype=torch.uint8), np.zeros((8, 16), dtype=np.uint8)):
        with pytest.raises(ValueError, match="count must be"):
            lrp.compose_cameras([mk(None)], out, 2, 2, count=bad)
        with pytest.raises(ValueError, match="coverage must be"):
            lrp.compose_cameras([mk(None)], out, 2, 2, coverage=bad)
    with pytest.raises(ValueError, match="at most 5"):
        lrp.Camera.brown(8, 8, None, 6.0, 6.0, 3.5, 3.5, k=(0.0,) * 6)
