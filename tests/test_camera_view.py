"""CPU: a calibrated camera as the target (include/lrp.h "calibrated camera as the target") without a GPU —
lrp_camera_unproject, the host evaluation of the function the kernel calls, against the CPU model the GPU tests compare with
(tests/native/camera_view_model.c) bit for bit; that model against a float64 Newton iteration run to convergence, written here
in numpy; the pinhole target pinned to the existing rectilinear lens; +inf limits and NaN; the error tables, each error before
any device call; and the rule that the scenes of tests/camera_view_cases.py discriminate."""
import ctypes
import math

import numpy as np
import pytest

import camera_cases as cam
import camera_model as cmodel
import camera_view_cases as cvc
import camera_view_model as cvmodel
import cases
import coverage_cases as cc

# The bound tests/test_camera.py uses for the forward mapping at these sizes: binary32 against float64, in pixels.
COORD_TOL_PX = 1e-3
# has_ray of the model and of float64 may differ only where the float64 r2 / theta lies this close (relative) to limit ...
LIMIT_BAND = 1e-4
# ... and that may set aside at most this part of a camera's sub-samples
LIMIT_BAND_SHARE = 0.01
NAMES = list(cvc.TARGETS)


# ------------------------------------------------------------------ 1. the host entry point against the model, bit for bit
@pytest.mark.parametrize("name", NAMES)
def test_unproject_is_the_model_bit_for_bit(lrp, name):
    """Every sub-sample (n = 3) of every target camera: rays and has_ray of lrp_camera_unproject == the model's."""
    T = cvc.target(lrp, name)
    uv = cvc.sub_positions(T["size"], 3)
    m_uv, m_ray, m_has = cvmodel.detail(T, 3)
    assert (m_uv == uv).all(), "the model's sub-sample positions"
    rays, has = lrp.camera_unproject(cam.product(lrp, T), uv.reshape(-1, 2))
    assert rays.dtype == np.float32 and rays.shape == (uv.size // 2, 3) and has.dtype == bool
    assert (has == m_has.ravel()).all(), f"{name}: has_ray"
    cases.assert_same_bits(rays, m_ray.reshape(-1, 3), f"{name}: rays")
    again, has2 = cvmodel.unproject(T, uv.reshape(-1, 2))
    cases.assert_same_bits(again, rays, f"{name}: camview_unproject")
    assert (has2 == has).all()
    print(f"{name}: {has.size} sub-samples, {int(has.sum())} with a ray")
    if name in cvc.CLIPPED:
        assert has.any() and not has.all()
    else:
        assert has.all()
    if T["model"] == cam.BROWN:
        assert (rays[has][:, 2] == -1.0).all()
    else:
        assert np.abs(np.linalg.norm(rays[has].astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_n1_positions_are_the_pixel_centres():
    uv = cvc.sub_positions((33, 9), 1)
    ys, xs = np.mgrid[0:9, 0:33]
    assert (uv[:, :, 0, 0] == xs).all() and (uv[:, :, 0, 1] == ys).all()


# ------------------------------------------------------------------ 2. the model against float64
@pytest.mark.parametrize("name", NAMES)
def test_model_against_float64(lrp, name):
    """The 8-step binary32 inverse against numpy float64 Newton run to convergence (80 steps, the same sticky rule): the ray,
    projected forward in float64, lands within 1e-3 px of the sub-sample wherever both have a ray; has_ray agrees everywhere
    but within a relative 1e-4 of limit."""
    T = cvc.target(lrp, name)
    uv, ray, has = (a.reshape(-1, a.shape[-1]) if a.ndim == 4 else a.ravel() for a in cvmodel.detail(T, 3))
    ray64, has64, q64 = cvc.unproject64(T, uv)
    both = has & has64
    assert both.any()
    back = cam.project64(T, ray[both].astype(np.float64))
    err = np.abs(back - uv[both].astype(np.float64)).max()
    limit = float(np.float32(T["limit"]))
    with np.errstate(invalid="ignore"):
        band = np.abs(q64 - limit) <= LIMIT_BAND * limit if math.isfinite(limit) else np.zeros_like(has)
    differ = has != has64
    print(f"{name}: {has.size} sub-samples, {int(both.sum())} with a ray in both, round trip {err:.3g} px, "
          f"has_ray differs on {int(differ.sum())} ({int((differ & ~band).sum())} outside the band), band {int(band.sum())}")
    assert err <= COORD_TOL_PX
    assert not (differ & ~band).any()
    assert band.mean() <= LIMIT_BAND_SHARE
    # and the rays themselves agree (a direction: compare after normalising)
    unit = lambda r: r / np.linalg.norm(r, axis=1, keepdims=True)
    assert np.abs(unit(ray[both].astype(np.float64)) - unit(ray64[both])).max() < 1e-5


# ------------------------------------------------------------------ 3. the pinhole target is the rectilinear lens
def test_pinhole_target_is_the_rectilinear_lens(lrp):
    """A target with k = 0, cx = w / 2 - 0.5, cy = h / 2 - 0.5, fx = w / sensor_width * focal: sx, sy of a source camera behind
    it against sx, sy behind the rectilinear target of the camera model."""
    w, h = 64, 48
    lens = cc.lens(lrp, "rect18", w, h)
    T = cam.camera(cam.BROWN, (w, h), w / lens.sensor_width * 18.0, h / lens.sensor_height * 18.0, w / 2 - 0.5, h / 2 - 0.5, (0.0,) * 5, cam.INF)
    S = cam.resolve(lrp, cam.RIG[0])
    rot = np.asarray(cases.rotation(lrp, cam.RIG_ROTATIONS[0]), dtype=np.float32).reshape(3, 3)
    for n in (1, 3):
        _, ray, has = cvmodel.detail(T, n)
        assert has.all()
        _, want, imaged, _ = cmodel.detail(S, lens, w, h, n, rot)
        r = ray.reshape(-1, 3)
        turned = np.stack([rot[j, 0] * r[:, 0] + rot[j, 1] * r[:, 1] + rot[j, 2] * r[:, 2] for j in range(3)], axis=1)
        sxy, imaged2 = cmodel.project(S, turned)
        near = imaged.ravel() & imaged2
        assert near.mean() > 0.5
        err = np.abs(sxy[near].astype(np.float64) - want.reshape(-1, 2)[near]).max()
        print(f"n {n}: {int(near.sum())} sub-samples, largest difference {err:.3g} px")
        assert err <= COORD_TOL_PX


# ------------------------------------------------------------------ 4. +inf limits and NaN
def test_infinite_limit_and_nan(lrp):
    """limit = +inf is legal, and then ok rests on NaN alone; a step with det == 0 (gp == 0) gives has_ray false or a finite ray,
    never a NaN ray with has_ray true."""
    wide = cvc.target(lrp, "brown_wide")
    uv = cvc.sub_positions(wide["size"], 2).reshape(-1, 2)
    rays, has = lrp.camera_unproject(cam.product(lrp, wide), uv)
    rays_inf, has_inf = lrp.camera_unproject(cam.product(lrp, dict(wide, limit=cam.INF)), uv)
    assert has.all() and has_inf.all()
    cases.assert_same_bits(rays_inf, rays, "limit = +inf inside the domain")
    # BROWN, k = 0, p2 = -1/6: at X, Y = 1, 0 jxx = 1 + 6 p2 = 0 and jxy = 0, so det == 0 in the first step.  FISHEYE,
    # k1 = -1/3: gp == 0 at theta = 1.  Both sit at the principal point + (fx, 0); a grid of positions round it.
    f = np.float32
    grid = np.stack(np.meshgrid(np.arange(-2, 2.25, 0.25, dtype=f) + f(4.0), np.arange(-2, 2.25, 0.25, dtype=f) + f(4.0)), axis=-1).reshape(-1, 2)
    assert (grid == np.array([5.0, 4.0], dtype=f)).all(axis=1).any()
    for c in (cam.camera(cam.BROWN, (8, 8), 1.0, 1.0, 4.0, 4.0, (0.0, 0.0, 0.0, float(f(-1.0) / f(6.0)), 0.0), limit=cam.INF),
              cam.camera(cam.FISHEYE, (8, 8), 1.0, 1.0, 4.0, 4.0, (float(f(-1.0) / f(3.0)), 0.0, 0.0, 0.0), limit=cam.INF),
              cam.camera(cam.BROWN, (8, 8), 1.0, 1.0, 4.0, 4.0, (-0.5, 0.0, 0.0, 0.0, 0.0), limit=cam.INF),
              cam.camera(cam.FISHEYE, (8, 8), 1.0, 1.0, 4.0, 4.0, (0.0,) * 4, limit=cam.INF)):
        with np.errstate(all="ignore"):
            rays, has = lrp.camera_unproject(cam.product(lrp, c), grid)
            m_rays, m_has = cvmodel.unproject(c, grid)
        cases.assert_same_bits(rays, m_rays, "det == 0")
        assert (has == m_has).all() and has.any()
        assert np.isfinite(rays[has]).all(), "a ray that is not finite with has_ray true"
        at = (grid == np.array([5.0, 4.0], dtype=f)).all(axis=1)
        print(f"model {c['model']} k {c['k']}: {int(has.sum())} of {has.size} with a ray; at the singular position has_ray {bool(has[at][0])}, ray {rays[at][0]}")


# ------------------------------------------------------------------ 5. argument errors (no device is touched before them)
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


def _call(lrp, cams, target, n=2, mode=0, interp=2, channels=4, out_data=0x2000, null_cams=False):
    lib = lrp._native.load()
    k = len(cams)
    arr = (lrp._native.LrpCamera * max(k, 1))(*cams)
    st = lib.lrp_camera_view_device(None if null_cams else arr, k, None, None if target is None else ctypes.byref(target), out_data, channels, n,
                                    interp, mode, None, None, None, -1, None)
    return st, lib.lrp_last_error().decode()


def test_argument_errors(lrp):
    S = lrp.Status
    good, fish = _good(lrp), _good(lrp, 1)
    tgt = _with(good, data=None)  # the target's data is ignored
    nan, inf = math.nan, math.inf
    # good calls get as far as the device: both target models, mixed sources, every n and mode
    for n in range(1, 16):
        assert _call(lrp, [good, fish, good], _with(fish if n % 2 else good, data=None), n=n, mode=n % 3, interp=n % 3)[0] == S.NO_DEVICE
    assert _call(lrp, [good], _with(tgt, limit=inf))[0] == S.NO_DEVICE and _call(lrp, [good], _with(tgt, limit=0.0))[0] == S.NO_DEVICE
    assert _call(lrp, [good] * 8, tgt)[0] == S.NO_DEVICE
    bad_tgt, bad_cam = _with(tgt, model=5), _with(good, model=5)
    # 1. n_in, mode — before anything else
    for k in (0, 9):
        st, text = _call(lrp, [good] * k, None, n=16, interp=7)
        assert st == S.BAD_ARG and "n_in" in text
    st, text = _call(lrp, [good], None, mode=3, null_cams=True)
    assert st == S.BAD_ARG and "mode" in text
    # 2. NULL, before the target
    for kw in (dict(null_cams=True), dict(out_data=None)):
        assert _call(lrp, [good], bad_tgt, interp=7, channels=0, **kw)[0] == S.NULL
    assert _call(lrp, [good], None, interp=7, channels=0)[0] == S.NULL
    # 3. the target, before channels, the interpolation and the cameras; within it model, size, values
    late = dict(interp=7, channels=0, n=0)
    st, text = _call(lrp, [bad_cam], _with(bad_tgt, width=0, fx=nan), **late)
    assert st == S.BAD_ARG and text.startswith("target: ") and "model" in text
    for size in (dict(width=0), dict(height=-3)):
        st, text = _call(lrp, [bad_cam], _with(tgt, fx=nan, **size), **late)
        assert st == S.BAD_DIMS and text.startswith("target: ")
    st, text = _call(lrp, [bad_cam], _with(tgt, width=1 << 15, height=1 << 15, fx=nan), interp=7, n=0)  # 2^30 pixels of 4 channels
    assert st == S.BAD_DIMS and text.startswith("target: ")
    assert _call(lrp, [good], _with(tgt, width=1 << 15, height=1 << 14))[0] == S.NO_DEVICE  # 2^31 floats: the largest frame
    for field in ("fx", "fy", "cx", "cy"):
        for bad in (nan, inf, -inf):
            st, text = _call(lrp, [bad_cam], _with(tgt, **{field: bad}), **late)
            assert st == S.BAD_ARG and text.startswith("target: ") and field in text, (field, bad, text)
    for j in range(5):
        st, text = _call(lrp, [bad_cam], _with(tgt, **{f"k{j}": nan}), **late)
        assert st == S.BAD_ARG and text.startswith("target: ") and f"k[{j}]" in text
    fish_tgt = _with(fish, data=None)
    for j in range(4):
        st, text = _call(lrp, [bad_cam], _with(fish_tgt, **{f"k{j}": -inf}), **late)
        assert st == S.BAD_ARG and text.startswith("target: ") and f"k[{j}]" in text
    assert _call(lrp, [good], _with(fish_tgt, k4=nan))[0] == S.NO_DEVICE  # FISHEYE ignores k[4]
    for field in ("fx", "fy"):
        for zero in (0.0, -0.0):
            st, text = _call(lrp, [bad_cam], _with(tgt, **{field: zero}), **late)
            assert st == S.BAD_ARG and text.startswith("target: ") and field in text
    for bad in (nan, -1.0, -inf):
        st, text = _call(lrp, [bad_cam], _with(tgt, limit=bad), **late)
        assert st == S.BAD_ARG and text.startswith("target: ") and "limit" in text
    # 4. channels, before the interpolation and the cameras
    for ch in (0, -1):
        assert _call(lrp, [bad_cam], tgt, interp=7, channels=ch, n=0)[0] == S.CHANNELS
    # 5. interpolation, before the cameras
    assert _call(lrp, [bad_cam], tgt, interp=7, n=0)[0] == S.INTERPOLATION and _call(lrp, [bad_cam], tgt, interp=-1)[0] == S.INTERPOLATION
    assert _call(lrp, [good], tgt, interp=3)[0] == S.INTERPOLATION  # no Lanczos-3
    # 6. per camera, ascending, as lrp_compose_cameras_device checks them
    st, text = _call(lrp, [good, bad_cam, _with(good, width=0)], tgt, n=0)
    assert st == S.BAD_ARG and "camera 1" in text and "model" in text
    st, text = _call(lrp, [good, _with(good, width=0, data=None), bad_cam], tgt, n=0)
    assert st == S.BAD_DIMS and "camera 1" in text
    st, text = _call(lrp, [_with(fish, width=1 << 15, height=1 << 15, data=None)], tgt)
    assert st == S.BAD_DIMS and "camera 0" in text
    st, text = _call(lrp, [good, good, _with(good, data=None, fx=nan)], tgt, n=0)
    assert st == S.NULL and "camera 2" in text
    st, text = _call(lrp, [good, _with(fish, cy=inf)], tgt, n=0)
    assert st == S.BAD_ARG and "camera 1" in text and "cy" in text
    st, text = _call(lrp, [_with(good, k4=nan)], tgt, n=0)
    assert st == S.BAD_ARG and "camera 0" in text and "k[4]" in text
    st, text = _call(lrp, [good, _with(fish, limit=nan)], tgt, n=0)
    assert st == S.BAD_ARG and "camera 1" in text and "limit" in text
    # 7. num_samples last
    for n in (0, -1, 16):
        st, text = _call(lrp, [good, fish], tgt, n=n)
        assert st == S.BAD_ARG and "num_samples" in text
    assert "lrp_camera_view_device" in lrp._native.SYMBOLS and "lrp_camera_unproject" in lrp._native.SYMBOLS
    assert lrp._native.load().lrp_abi_version() == 3


def test_unproject_errors(lrp):
    lib, S = lrp._native.load(), lrp.Status
    good = _good(lrp)
    uv, rays, has = (np.zeros((2, 2), dtype=np.float32), np.zeros((2, 3), dtype=np.float32), np.zeros(2, dtype=np.uint8))
    call = lambda c, u=uv, n=2, r=rays, h=has: lib.lrp_camera_unproject(None if c is None else ctypes.byref(c), None if u is None else u.ctypes.data,
                                                                        n, None if r is None else r.ctypes.data, None if h is None else h.ctypes.data)
    assert call(good) == S.OK and call(good, h=None) == S.OK and call(good, n=0) == S.OK
    assert call(_with(good, width=0, height=0, data=None)) == S.OK  # the size and the data are not looked at
    assert call(None) == S.NULL and call(good, u=None) == S.NULL and call(good, r=None) == S.NULL
    assert call(good, n=-1) == S.BAD_ARG and call(_with(good, model=2)) == S.BAD_ARG
    for bad in (dict(fx=math.nan), dict(cy=math.inf), dict(k4=math.nan), dict(fy=0.0), dict(limit=math.nan), dict(limit=-1.0)):
        assert call(_with(good, **bad)) == S.BAD_ARG, bad
    assert call(_with(good, limit=math.inf)) == S.OK and call(_with(_good(lrp, 1), k4=math.nan)) == S.OK


def test_tensors_are_checked_in_python(lrp):
    import torch

    mk = lambda data: lrp.Camera.brown(8, 8, data, 6.0, 6.0, 3.5, 3.5)
    tgt = lrp.Camera.fisheye(16, 8, None, 6.0, 6.0, 7.5, 3.5)
    for out in (np.zeros((8, 16, 4), dtype=np.float32), torch.zeros((8, 16, 4)), None):
        with pytest.raises(ValueError, match="out must be"):
            lrp.camera_view([mk(None)], tgt, out, 2, 2)


# ------------------------------------------------------------------ 6. the scenes of the GPU test discriminate
@pytest.mark.parametrize("name", NAMES)
def test_scenes_discriminate(lrp, name):
    T = cvc.target(lrp, name)
    cams, rots = cvc.rig(lrp)
    srcs = cam.sources(cams, channels=1)
    for n in (2, 3):
        out, count, m = cvmodel.compose(cams, srcs, T, n, 0, rots, 1)
        _, _, has = cvmodel.detail(T, n)
        print(f"{name} n {n}: m == 0 {int((m == 0).sum())}, partial {int(((m > 0) & (m < n * n)).sum())}, full {int((m == n * n).sum())}, "
              f"count >= 2 {int((count >= 2).sum())}, sub-samples without a ray {int((~has).sum())} of {has.size}")
        assert cam.discriminates(count, m, n)
        assert (m <= has.sum(axis=2)).all() and ((out.view(np.uint32) == 0).all(axis=2) == (m == 0)).all()
        if name in cvc.CLIPPED:
            assert has.any() and not has.all()
            part = has.any(axis=2) & ~has.all(axis=2)  # pixels through which the edge of the domain runs
            assert part.any() and (m[part] < n * n).all()
    if name == "brown_clipped":
        # the polynomial turns at r = 1.86, which it images at r_d = 1.137: a disc of 18.2 px at fx = 16, 60 % of the 48 x 36 frame
        assert 0.35 < 1.0 - has.mean() < 0.45, "about 40 % of the frame has no ray"
        for n in (1, 15):
            _, count, m = cvmodel.compose(cams, srcs, T, n, 0, rots, 1)
            assert (m == 0).any() and (m == n * n).any() and (count >= 2).any() and (n == 1 or ((m > 0) & (m < n * n)).any())
