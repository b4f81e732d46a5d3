"""CPU: exposure matching across a camera rig (include/lrp.h "exposure matching across a camera rig").  The
CPU model of tests/camera_gain_model.py against the definition rebuilt in numpy from the existing camera model, lrp_camera_gains
against numpy's solver, recovery of known exposures, gains of 1.0f against the model of lrp_compose_cameras_device byte for byte,
both error tables — and the rule that the scenes of tests/test_gpu_camera_gain.py discriminate.  No device is touched."""
import ctypes
import math

import numpy as np
import pytest

import camera_cases as cam
import camera_gain_cases as gc
import camera_gain_model as gmodel
import camera_model as cmodel
import cases

F32 = np.float32


@pytest.fixture(autouse=True)
def extensions_on(lrp):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    try:
        yield
    finally:
        lrp.lens_extensions(prev)


def definition(cams, srcs, lout, ow, oh, rots, lo, hi):
    """The statistic rebuilt from one bilinear n = 1 render and coverage plane per camera (the existing camera model): the table,
    and per camera the coverage, the validity and Y."""
    C = srcs[0].shape[2]
    cov, valid, q, lum = [], [], [], []
    for i, (c, s) in enumerate(zip(cams, srcs)):
        img, _, m = cmodel.compose([c], [s], lout, ow, oh, 1, 1, None if rots is None else [rots[i]])
        with np.errstate(all="ignore"):
            Y = img[..., 0] if C < 3 else (F32(0.25) * img[..., 0] + F32(0.5) * img[..., 1]) + F32(0.25) * img[..., 2]
            assert Y.dtype == np.float32
            ok = (m == 1) & (Y >= F32(lo)) & (Y <= F32(hi))
            qi = np.where(ok, Y * F32(65536.0), F32(0.0))
        assert qi.dtype == np.float32  # (the product is exact: a power of two; the conversion truncates)
        cov.append(m == 1), valid.append(ok), q.append(np.trunc(qi).astype(np.int64)), lum.append(Y)
    table = np.zeros((8, 8, 2), dtype=np.int64)
    for i in range(len(cams)):
        for j in range(len(cams)):
            both = valid[i] & valid[j]
            table[i, j] = int(both.sum()), int(q[i][both].sum())
    return table, cov, valid, lum


# ------------------------------------------------------------------ 1. the scenes discriminate
@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_rig_scenes_discriminate(lrp, out_name):
    lout, cams, rots = cam.rig(lrp, out_name)
    ow, oh = cam.OUT_SIZE
    srcs = cam.sources(cams)
    lo, hi = gc.RANGE[out_name]
    table, cov, valid, _ = definition(cams, srcs, lout, ow, oh, rots, lo, hi)
    pairs = 0
    for i, j in ((0, 1), (0, 2), (1, 2)):
        both_cover, both_valid = int((cov[i] & cov[j]).sum()), int(table[i, j, 0])
        print(f"{out_name} pair {i}{j}: both cover {both_cover}, both valid {both_valid}")
        if both_valid > 0:
            pairs += 1
            assert both_valid < both_cover, "the range excludes none of the pixels both cameras cover"
    assert pairs >= 2
    if out_name in gc.MEASURED:
        assert [(int((cov[i] & cov[j]).sum()), int(table[i, j, 0])) for i, j in ((0, 1), (0, 2), (1, 2))] == gc.MEASURED[out_name]


def test_eight_cameras_have_zero_and_non_zero_overlaps(lrp):
    lout, cams, rots, srcs = gc.eight_scene(lrp)
    table = gmodel.overlap(cams, srcs, lout, 80, 48, rots, *gc.RANGE["eight"])
    off = table[..., 0][~np.eye(8, dtype=bool)]
    assert (off == 0).any() and (off > 0).any() and (np.diagonal(table[..., 0]) > 0).all()


# ------------------------------------------------------------------ 2. the model's statistic is the definition
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_model_statistic_is_the_definition(lrp, out_name, channels):
    lout, cams, rots = cam.rig(lrp, out_name)
    ow, oh = cam.OUT_SIZE
    srcs = cam.sources(cams, channels)
    lo, hi = gc.RANGE[out_name]
    want = definition(cams, srcs, lout, ow, oh, rots, lo, hi)[0]
    got = gmodel.overlap(cams, srcs, lout, ow, oh, rots, lo, hi)
    assert got.dtype == np.int64 and (got == want).all(), (got[:3, :3], want[:3, :3])
    assert (got[..., 0] == got[..., 0].T).all() and (got[3:] == 0).all() and (got[:, 3:] == 0).all()


def test_model_statistic_eight_planted_and_no_rotations(lrp):
    lout, cams, rots, srcs = gc.eight_scene(lrp)
    lo, hi = gc.RANGE["eight"]
    assert (gmodel.overlap(cams, srcs, lout, 80, 48, rots, lo, hi) == definition(cams, srcs, lout, 80, 48, rots, lo, hi)[0]).all()
    lout, cams, rots = cam.rig(lrp, "eqr_part")
    planted = cam.sources(cams, 4, planted=True)
    want, _, valid, lum = definition(cams, planted, lout, 80, 48, rots, 0.0, 32768.0)
    assert (gmodel.overlap(cams, planted, lout, 80, 48, rots, 0.0, 32768.0) == want).all()
    with np.errstate(all="ignore"):
        bad = [np.isnan(Y) | np.isinf(Y) | (Y > 32768.0) | (Y < 0) for Y in lum]
    assert any(b.any() for b in bad) and not any((b & v).any() for b, v in zip(bad, valid)), "NaN, infinities, 3e38 and negatives are invalid"
    lout, cams, _ = cam.rig(lrp, "eqr_full")
    srcs = cam.sources(cams)
    want = definition(cams, srcs, lout, 80, 48, None, 0.6, 0.9)[0]
    assert (gmodel.overlap(cams, srcs, lout, 80, 48, None, 0.6, 0.9) == want).all() and want[0, 1, 0] > 0


# ------------------------------------------------------------------ 3. lrp_camera_gains
def normal_equations(table, active, sigma_n, sigma_g):
    """A, b of include/lrp.h in float64 over the cameras `active`, and I."""
    N = table[..., 0].astype(np.float64)
    with np.errstate(all="ignore"):
        I = np.where(N > 0, table[..., 1].astype(np.float64) / (65536.0 * np.where(N > 0, N, 1.0)), 0.0)
    sn2, sg2 = float(F32(sigma_n)) ** 2, float(F32(sigma_g)) ** 2
    m = len(active)
    A, b = np.zeros((m, m)), np.zeros(m)
    for r, k in enumerate(active):
        for c, j in enumerate(active):
            A[r, r] += N[k, j] / sg2
            b[r] += N[k, j] / sg2
            if j != k:
                A[r, r] += 2.0 * N[k, j] * I[k, j] ** 2 / sn2
                A[r, c] = -2.0 * N[k, j] * I[k, j] * I[j, k] / sn2
    return A, b, N, I


def energy(g, N, I, sigma_n, sigma_g):
    sn2, sg2 = float(F32(sigma_n)) ** 2, float(F32(sigma_g)) ** 2
    n = len(g)
    return 0.5 * sum(N[i, j] * ((g[i] * I[i, j] - g[j] * I[j, i]) ** 2 / sn2 + (1.0 - g[i]) ** 2 / sg2) for i in range(n) for j in range(n))


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def gain_tables(lrp):
    out = []
    for out_name in ("rect18", "eqr_part"):
        lout, cams, rots = cam.rig(lrp, out_name)
        srcs = [s * F32(e) for s, e in zip(cam.sources(cams), (0.8, 1.0, 1.3))]
        out.append((3, gmodel.overlap(cams, srcs, lout, 80, 48, rots, 0.3, 1.4)))
    lout, cams, rots, srcs = gc.eight_scene(lrp)
    srcs = [s * F32(0.7 + 0.1 * i) for i, s in enumerate(srcs)]
    out.append((8, gmodel.overlap(cams, srcs, lout, 80, 48, rots, 0.2, 2.0)))
    return out


def test_gains_against_numpy(lrp):
    for n, table in gain_tables(lrp):
        for sigma_n, sigma_g in ((10 / 255, 0.1), (0.02, 0.5)):
            got = lrp.camera_gains(table, n, sigma_n, sigma_g)
            assert got.dtype == np.float32 and got.shape == (n,)
            A, b, N, I = normal_equations(table, list(range(n)), sigma_n, sigma_g)
            assert np.linalg.cond(A) < 1e6 and (np.diagonal(A) > 0).all() and (A[~np.eye(n, dtype=bool)] <= 0).all() and (b >= 0).all()
            assert (np.linalg.eigvalsh((A + A.T) / 2) > 0).all()
            want = np.linalg.solve(A, b)
            print(f"n {n} sigma {sigma_n:.4f} {sigma_g}: gains {got}, cond {np.linalg.cond(A):.1f}")
            assert (ulps(got, want.astype(np.float32)) <= 1).all() and (got > 0).all()
            # the gradient of e at the solution, by central differences (e is quadratic: they are exact up to rounding).  The stored
            # gains are the solution rounded to binary32, so the gradient A (g - g*) is at most |A|_inf * 2^-24 * max g.
            g = got.astype(np.float64)
            h = 1e-3
            grad = np.array([(energy(g + h * np.eye(n)[k], N, I, sigma_n, sigma_g) - energy(g - h * np.eye(n)[k], N, I, sigma_n, sigma_g)) / (2 * h)
                             for k in range(n)])
            grad1 = A @ np.ones(n) - b
            bound = np.abs(A).sum(axis=1).max() * 2.0 ** -24 * g.max()
            print(f"  gradient at the solution {np.abs(grad).max():.3e} (bound {bound:.3e}), at g = 1 {np.abs(grad1).max():.3e}")
            assert np.abs(grad).max() <= 1.01 * bound + 1e-9 * np.abs(grad1).max() and np.abs(grad).max() < 1e-5 * np.abs(grad1).max()
    # the defaults are OpenCV's
    n, table = gain_tables(lrp)[0]
    assert (lrp.camera_gains(table, n) == lrp.camera_gains(table, n, 10 / 255, 0.1)).all()
    import torch

    assert (lrp.camera_gains(torch.from_numpy(table), n) == lrp.camera_gains(table, n)).all()


def test_gains_camera_without_a_valid_pixel(lrp):
    n, table = gain_tables(lrp)[2]
    for dead in (0, 3, 7):
        t = table.copy()
        t[dead, :, :] = 0
        t[:, dead, :] = 0
        got = lrp.camera_gains(t, n)
        assert got[dead].view(np.uint32) == F32(1.0).view(np.uint32)
        active = [k for k in range(n) if k != dead]
        A, b, _, _ = normal_equations(t, active, 10 / 255, 0.1)
        assert (ulps(got[active], np.linalg.solve(A, b).astype(np.float32)) <= 1).all()
        # ... and equal the call on the table with that camera removed
        small = np.zeros_like(t)
        small[:7, :7] = t[np.ix_(active, active)]
        assert (lrp.camera_gains(small, 7) == got[active]).all()
    assert (lrp.camera_gains(np.zeros((8, 8, 2), dtype=np.int64), 5) == np.ones(5, dtype=np.float32)).all()


def test_equal_intensities_give_unit_gains(lrp):
    rng = np.random.default_rng(5)
    for n in (1, 3, 8):
        t = np.zeros((8, 8, 2), dtype=np.int64)
        N = rng.integers(0, 900, (n, n))
        N = np.triu(N) + np.triu(N, 1).T + np.diag(np.full(n, 1000))
        t[:n, :n, 0] = N
        t[:n, :n, 1] = N * int(0.625 * 65536)  # I_ij = 0.625 in every overlap
        got = lrp.camera_gains(t, n)
        assert (ulps(got, np.ones(n, dtype=np.float32)) <= 1).all(), got


# ------------------------------------------------------------------ 4. recovery
def test_recovery_of_known_exposures(lrp):
    """Three frames cut from one smooth world and scaled by 0.7, 1.0 and 1.4: g_i * e_i agree to within the bound (twice the spread
    measured with this model: DESIGN.md section 19), and inside the overlaps neighbouring cameras' gained contributions differ
    less than the plain ones."""
    lout, cams, rots, srcs = gc.recovery_scene(lrp)
    ow, oh = cam.OUT_SIZE
    table = gmodel.overlap(cams, srcs, lout, ow, oh, rots, 0.02, 8.0)
    assert all(table[i, j, 0] > 100 for i, j in ((0, 1), (0, 2), (1, 2)))
    before = max(gc.EXPOSURES) / min(gc.EXPOSURES) - 1.0
    for (sigma_n, sigma_g), measured in gc.RECOVERY_SPREAD_MEASURED.items():
        g = lrp.camera_gains(table, 3, sigma_n, sigma_g)
        prod = g.astype(np.float64) * np.array(gc.EXPOSURES)
        spread = prod.max() / prod.min() - 1.0
        print(f"sigma_g {sigma_g}: gains {g}, g * e {prod}, spread {spread:.3e} (without gains {before:.3f}; measured {measured}, bound {2 * measured})")
        assert spread <= 2 * measured and spread < before
    gains = lrp.camera_gains(table, 3)
    # FEATHER: camera i's contribution is g_i * s_i; one camera alone under FEATHER is w * (g * s) / w
    ones = np.ones(3, dtype=np.float32)
    diffs = {}
    for name, g in (("plain", ones), ("gained", gains)):
        part = [gmodel.compose([c], [s], [g[i]], lout, ow, oh, 1, 1, [rots[i]], 2) for i, (c, s) in enumerate(zip(cams, srcs))]
        total, count = 0.0, 0
        for i, j in ((0, 1), (0, 2), (1, 2)):
            both = (part[i][2] == 1) & (part[j][2] == 1)
            total += float(np.abs(part[i][0][both][:, :3].astype(np.float64) - part[j][0][both][:, :3]).sum())
            count += 3 * int(both.sum())
        diffs[name] = total / count
    print(f"mean |contribution_i - contribution_j| inside the overlaps: plain {diffs['plain']:.5f}, gained {diffs['gained']:.5f}")
    assert diffs["gained"] < diffs["plain"]


# ------------------------------------------------------------------ 5. gains of 1.0f are lrp_compose_cameras_device
@pytest.mark.parametrize("channels", [1, 3, 4, 11])
def test_unit_gains_reproduce_the_camera_model(lrp, channels):
    lout, cams, rots = cam.rig(lrp, "eqr_part")
    srcs = cam.sources(cams, channels, planted=True)
    ones = np.ones(3, dtype=np.float32)
    seen_special = False
    for n, interp, mode, post in ((2, 1, 0, None), (2, 1, 1, None), (3, 2, 2, None), (1, 0, 1, (2.0, 3.0)), (2, 1, 2, (2.0, 3.0))):
        want = cmodel.compose(cams, srcs, lout, 80, 48, n, interp, rots, mode, post)
        got = gmodel.compose(cams, srcs, ones, lout, 80, 48, n, interp, rots, mode, post)
        cases.assert_same_bits(got[0], want[0], f"C {channels} n {n} interp {interp} mode {mode} post {post}")
        assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
        seen_special |= bool(np.isnan(want[0]).any() and np.isinf(want[0]).any())
    assert seen_special and any(np.signbit(s[s == 0]).any() for s in srcs)


def test_gains_multiply_colour_only(lrp):
    """The gained model against the camera model on pre-multiplied frames: FIRST with nearest is a copy, so g * s is the whole
    arithmetic — and channels 3 .. are untouched."""
    lout, cams, rots = cam.rig(lrp, "eqr_part")
    g = np.array(gc.GAINS, dtype=np.float32)
    for channels in (1, 2, 4, 11):
        srcs = cam.sources(cams, channels)
        scaled = [s.copy() for s in srcs]
        for s, gi in zip(scaled, g):
            s[..., :3] = gi * s[..., :3]
        want = cmodel.compose(cams, scaled, lout, 80, 48, 1, 0, rots, 0)
        got = gmodel.compose(cams, srcs, g, lout, 80, 48, 1, 0, rots, 0)
        cases.assert_same_bits(got[0], want[0], f"C {channels}")
        plain = cmodel.compose(cams, srcs, lout, 80, 48, 2, 1, rots, 2)[0]
        gained = gmodel.compose(cams, srcs, g, lout, 80, 48, 2, 1, rots, 2)[0]
        cases.assert_same_bits(gained[..., 3:], plain[..., 3:], f"C {channels}: channels beyond the colour")
        assert (~cases.same_bits(gained[..., :3], plain[..., :3])).any()


# ------------------------------------------------------------------ 6. the error tables, in order, without a device
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


def _out(lrp, lout=None, out_channels=4, out_size=(8, 8), out_data=0x2000):
    cout = lrp.Image(lout or lrp.LensInfo.equirectangular(), out_size[0], out_size[1], out_channels, None).to_c()
    cout.data = out_data
    return cout


def _overlap(lrp, cams, lo=0.02, hi=0.98, stats=0x3000, null_cams=False, null_out=False, **out):
    lib = lrp._native.load()
    k = len(cams)
    arr = (lrp._native.LrpCamera * max(k, 1))(*cams)
    cout = _out(lrp, **out)
    st = lib.lrp_camera_overlap_device(None if null_cams else arr, k, None, None if null_out else ctypes.byref(cout), lo, hi, stats, -1, None)
    return st, lib.lrp_last_error().decode()


def _gain(lrp, cams, gains=(), n=2, mode=0, interp=2, null_cams=False, null_out=False, null_gains=False, **out):
    lib = lrp._native.load()
    k = len(cams)
    arr = (lrp._native.LrpCamera * max(k, 1))(*cams)
    cout = _out(lrp, **out)
    g = np.ones(max(k, 1), dtype=np.float32)
    g[:len(gains)] = gains
    st = lib.lrp_compose_cameras_gain_device(None if null_cams else arr, k, None, None if null_gains else g.ctypes.data,
                                             None if null_out else ctypes.byref(cout), n, interp, mode, None, None, None, -1, None)
    return st, lib.lrp_last_error().decode()


def test_overlap_argument_errors(lrp):
    S, L = lrp.Status, lrp.LensInfo
    good, fish = _good(lrp), _good(lrp, 1)
    nan, inf = math.nan, math.inf
    bad_cam = _with(good, model=5)
    # good calls get as far as the device; out->data may be NULL; the ends of the range are allowed
    assert _overlap(lrp, [good, fish, good])[0] == S.NO_DEVICE and _overlap(lrp, [good] * 8, out_data=None)[0] == S.NO_DEVICE
    assert _overlap(lrp, [good], lo=0.0, hi=32768.0)[0] == S.NO_DEVICE and _overlap(lrp, [good], lo=0.5, hi=0.5)[0] == S.NO_DEVICE
    assert _overlap(lrp, [good], lo=-0.0, hi=0.0)[0] == S.NO_DEVICE
    # 1. n_in first
    for k in (0, 9):
        st, text = _overlap(lrp, [good] * k, null_out=True, stats=None, lo=nan)
        assert st == S.BAD_ARG and "n_in" in text
    # 2. NULL
    assert _overlap(lrp, [good], null_cams=True, out_channels=0)[0] == S.NULL and _overlap(lrp, [good], null_out=True, stats=None)[0] == S.NULL
    # 3. the output side, before the cameras; data is exempt
    lrp.lens_extensions(0)
    assert _overlap(lrp, [bad_cam], lout=L.stereographic(10.0, 36.0, 8, 8), out_channels=0)[0] == S.OUTPUT_LENS
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    assert _overlap(lrp, [good], lout=L.stereographic(10.0, 36.0, 8, 8))[0] == S.NO_DEVICE
    assert _overlap(lrp, [bad_cam], out_channels=0, out_size=(0, 8))[0] == S.CHANNELS
    assert _overlap(lrp, [bad_cam], out_size=(0, 8))[0] == S.BAD_DIMS
    assert _overlap(lrp, [bad_cam], out_size=(1 << 15, 1 << 15), out_data=None)[0] == S.BAD_DIMS
    # 5. per camera, ascending; before stats and the range
    st, text = _overlap(lrp, [good, bad_cam, _with(good, width=0)], stats=None, lo=nan, out_data=None)
    assert st == S.BAD_ARG and "camera 1" in text and "model" in text
    st, text = _overlap(lrp, [good, _with(good, width=0, data=None)], stats=None)
    assert st == S.BAD_DIMS and "camera 1" in text
    st, text = _overlap(lrp, [good, good, _with(good, data=None, fx=nan)], stats=None)
    assert st == S.NULL and "camera 2" in text
    st, text = _overlap(lrp, [good, _with(fish, fy=inf)], stats=None)
    assert st == S.BAD_ARG and "camera 1" in text and "fy" in text
    st, text = _overlap(lrp, [_with(fish, limit=-1.0)], stats=None)
    assert st == S.BAD_ARG and "limit" in text
    # then stats, then the range
    st, text = _overlap(lrp, [good], stats=None, lo=nan)
    assert st == S.NULL and "stats" in text
    for lo, hi in ((nan, 0.5), (0.1, nan), (-inf, 0.5), (0.1, inf), (-1e-9, 0.5), (0.6, 0.5), (0.5, 32768.5), (40000.0, 50000.0)):
        st, text = _overlap(lrp, [good, fish], lo=lo, hi=hi)
        assert st == S.BAD_ARG and "lo" in text, (lo, hi)
    for name in ("lrp_camera_overlap_device", "lrp_camera_gains", "lrp_compose_cameras_gain_device"):
        assert name in lrp._native.SYMBOLS
    assert lrp._native.load().lrp_abi_version() == 3


def test_gain_compose_argument_errors(lrp):
    S, L = lrp.Status, lrp.LensInfo
    good, fish = _good(lrp), _good(lrp, 1)
    nan, inf = math.nan, math.inf
    bad_cam = _with(good, model=5)
    for n in range(1, 16):
        assert _gain(lrp, [good, fish, good], (0.5, 0.0, 7.0), n=n, mode=n % 3, interp=n % 3)[0] == S.NO_DEVICE
    assert _gain(lrp, [good], (-0.0,))[0] == S.NO_DEVICE
    # 1. n_in, mode
    for k in (0, 9):
        st, text = _gain(lrp, [good] * k, n=16, interp=7, null_out=True, null_gains=True)
        assert st == S.BAD_ARG and "n_in" in text
    st, text = _gain(lrp, [good], mode=3, null_cams=True)
    assert st == S.BAD_ARG and "mode" in text
    # 2. NULL: cams, out, gains — before the output side
    assert _gain(lrp, [good], null_cams=True, interp=7)[0] == S.NULL and _gain(lrp, [good], null_out=True, interp=7)[0] == S.NULL
    st, text = _gain(lrp, [bad_cam], null_gains=True, interp=7, out_channels=0)
    assert st == S.NULL and "gains" in text
    # 3. the output side
    lrp.lens_extensions(0)
    assert _gain(lrp, [bad_cam], lout=L.stereographic(10.0, 36.0, 8, 8), interp=7, out_channels=0)[0] == S.OUTPUT_LENS
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    assert _gain(lrp, [bad_cam], interp=7, out_channels=0, out_size=(0, 8))[0] == S.CHANNELS
    assert _gain(lrp, [bad_cam], interp=7, out_size=(0, 8), out_data=None)[0] == S.BAD_DIMS
    assert _gain(lrp, [bad_cam], interp=7, out_data=None)[0] == S.NULL
    # 4. interpolation, before the cameras
    assert _gain(lrp, [bad_cam], (nan,), interp=7, n=0)[0] == S.INTERPOLATION
    # 5. per camera, before the gains
    st, text = _gain(lrp, [good, bad_cam], (nan, nan), n=0)
    assert st == S.BAD_ARG and "camera 1" in text and "model" in text
    st, text = _gain(lrp, [good, _with(good, data=None)], (nan, nan), n=0)
    assert st == S.NULL and "camera 1" in text
    # the gains: after the cameras, before num_samples; the text names the camera
    for bad in (nan, inf, -inf, -1.0, -1e-30):
        st, text = _gain(lrp, [good, fish, good], (1.0, 1.0, bad), n=0)
        assert st == S.BAD_ARG and "camera 2" in text and "gain" in text, bad
    st, text = _gain(lrp, [good, fish], (nan, -1.0), n=0)
    assert "camera 0" in text
    # 6. num_samples last
    for n in (0, -1, 16):
        st, text = _gain(lrp, [good, fish], n=n)
        assert st == S.BAD_ARG and "num_samples" in text


def test_camera_gains_argument_errors(lrp):
    S = lrp.Status
    lib = lrp._native.load()
    table = np.zeros(128, dtype=np.uint64)
    out = np.zeros(8, dtype=np.float32)
    call = lambda stats, n, sn, sg, g: lib.lrp_camera_gains(stats, n, sn, sg, g)
    assert call(table.ctypes.data, 8, 0.04, 0.1, out.ctypes.data) == S.OK and (out == 1.0).all()
    assert call(None, 0, math.nan, 0.1, out.ctypes.data) == S.NULL and call(table.ctypes.data, 0, math.nan, 0.1, None) == S.NULL
    for n in (0, 9, -1):
        assert call(table.ctypes.data, n, math.nan, 0.1, out.ctypes.data) == S.BAD_ARG and "n_in" in lib.lrp_last_error().decode()
    for sn, sg in ((0.0, 0.1), (-0.04, 0.1), (math.nan, 0.1), (math.inf, 0.1), (0.04, 0.0), (0.04, -1.0), (0.04, math.nan), (0.04, math.inf)):
        assert call(table.ctypes.data, 3, sn, sg, out.ctypes.data) == S.BAD_ARG and "sigma" in lib.lrp_last_error().decode()
    with pytest.raises(ValueError):
        lrp.camera_gains(np.zeros(100, dtype=np.int64), 3)
