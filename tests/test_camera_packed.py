"""CPU: lrp_compose_cameras_packed_device and lrp_camera_overlap_packed_device (include/lrp.h "calibrated cameras, packed
pixels") without a device — the symbols and their Python mirrors exist, the argument errors come in the documented order with
the documented statuses (all of them before a device is touched; valid arguments get as far as LRP_ERR_NO_DEVICE), the mirrors
refuse what they must before any pointer reaches the library, and every case of tests/camera_packed_cases.py discriminates on
the chain on the CPU (cpu_chain: numpy decode -> the model of tests/camera_gain_model.py -> numpy encode):
  - the planes: for n >= 2 camera_cases.discriminates(); for n == 1 pixels with m == 0, count == 1 and count >= 2;
  - the codes: among the samples of the covered pixels at least 64 distinct codes, and no code makes up more than a quarter;
  - the statistic under RANGE on decoded 8-bit noise: three pairs with N_ij > 0, and the range excludes at least a quarter of
    what both cameras cover.
The quarter-of-one-code condition under GAINS = (0.7, 1.0, 1.6) is derived, not tuned: of uniformly random bytes only camera
2's samples above code ~207 clamp to 255 under a gain of 1.6 — about a fifth of that camera's share under the nearest sampler,
fewer under the averaging ones."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import camera_cases as cam
import camera_packed_cases as kp

F32, F16, U8 = kp.F32, kp.F16, kp.U8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def extensions_on(lrp):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    try:
        yield
    finally:
        lrp.lens_extensions(prev)


def _good(lrp, model=0, size=(8, 8)):
    c = cam.product(lrp, cam.camera(model, size, 6.0, 6.0, 3.5, 3.5, (0.01, 0.001, 0.001, 0.001, 0.001), limit=1.0)).to_c()
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


def _compose(lrp, cams, gains=None, in_fmt=U8, in_pch=4, out_fmt=U8, out_pch=4, n=2, mode=0, interp=2, null_cams=False, null_out=False, **out):
    lib = lrp._native.load()
    k = len(cams)
    arr = (lrp._native.LrpCamera * max(k, 1))(*cams)
    cout = _out(lrp, **out)
    g = None
    if gains is not None:
        g = np.ones(max(k, 1), dtype=np.float32)
        g[:len(gains)] = gains
    st = lib.lrp_compose_cameras_packed_device(None if null_cams else arr, k, in_fmt, in_pch, None, None if g is None else g.ctypes.data,
                                               None if null_out else ctypes.byref(cout), out_fmt, out_pch, 255, n, interp, mode, None, None, None,
                                               -1, None)
    return st, lib.lrp_last_error().decode()


def _overlap(lrp, cams, in_fmt=U8, in_pch=4, lo=0.02, hi=0.98, stats=0x3000, null_cams=False, null_out=False, **out):
    lib = lrp._native.load()
    k = len(cams)
    arr = (lrp._native.LrpCamera * max(k, 1))(*cams)
    cout = _out(lrp, **out)
    st = lib.lrp_camera_overlap_packed_device(None if null_cams else arr, k, in_fmt, in_pch, None, None if null_out else ctypes.byref(cout), lo, hi,
                                              stats, -1, None)
    return st, lib.lrp_last_error().decode()


def test_symbols_and_python_mirrors_exist(lrp):
    lib = lrp._native.load()
    for name in ("lrp_compose_cameras_packed_device", "lrp_camera_overlap_packed_device"):
        assert hasattr(lib, name) and name in lrp._native.SYMBOLS
    assert lib.lrp_abi_version() == 3
    with open(os.path.join(ROOT, "include", "lrp.h")) as f:
        header = f.read()
    assert "int lrp_compose_cameras_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels," in header
    assert "int lrp_camera_overlap_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels," in header
    assert list(inspect.signature(lrp.compose_cameras_packed).parameters) == [
        "cameras", "in_format", "in_datas", "out_image", "out_format", "out_data", "out_fill", "num_samples", "interpolation", "rotation_matrices",
        "mode", "post", "count", "coverage", "device", "stream", "gains"]
    assert list(inspect.signature(lrp.camera_overlap_packed).parameters) == [
        "cameras", "in_format", "in_datas", "out_image", "rotation_matrices", "lo", "hi", "stats", "device", "stream"]
    sig = inspect.signature(lrp.camera_overlap_packed).parameters
    assert sig["lo"].default == 0.02 and sig["hi"].default == 0.98


def test_compose_argument_errors_in_the_documented_order(lrp):
    S, L = lrp.Status, lrp.LensInfo
    good, fish = _good(lrp), _good(lrp, 1)
    nan, inf = math.nan, math.inf
    bad_cam = _with(good, model=5)
    # valid arguments reach the device: both source formats, every output format, every sampler and mode, every n, gains or none
    for in_fmt in (F16, U8):
        for out_fmt in (F32, F16, U8):
            for interp in (0, 1, 2):
                assert _compose(lrp, [good, fish], in_fmt=in_fmt, out_fmt=out_fmt, interp=interp, mode=interp)[0] == S.NO_DEVICE
    for n in range(1, 16):
        assert _compose(lrp, [good, fish, good], (0.5, 0.0, 7.0), n=n)[0] == S.NO_DEVICE
    assert _compose(lrp, [good] * 8, (-0.0,), out_channels=8, in_pch=7, out_pch=64)[0] == S.NO_DEVICE
    # 1. n_in, mode — each of the parent's errors wins over a packed-format error (in_fmt F32 / 9, in_pch 0)
    for k in (0, 9):
        st, text = _compose(lrp, [good] * k, n=16, interp=7, null_out=True, in_fmt=F32)
        assert st == S.BAD_ARG and "n_in" in text
    st, text = _compose(lrp, [good], mode=3, null_cams=True, in_fmt=9)
    assert st == S.BAD_ARG and "mode" in text
    # 2. NULL
    assert _compose(lrp, [good], null_cams=True, interp=7, in_fmt=F32)[0] == S.NULL and _compose(lrp, [good], null_out=True, in_pch=0)[0] == S.NULL
    # 3. the output side
    lrp.lens_extensions(0)
    assert _compose(lrp, [bad_cam], lout=L.stereographic(10.0, 36.0, 8, 8), interp=7, out_channels=0, in_fmt=F32)[0] == S.OUTPUT_LENS
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    assert _compose(lrp, [bad_cam], interp=7, out_channels=0, out_size=(0, 8), in_fmt=F32)[0] == S.CHANNELS
    assert _compose(lrp, [bad_cam], interp=7, out_size=(0, 8), out_data=None, in_fmt=F32)[0] == S.BAD_DIMS
    assert _compose(lrp, [bad_cam], interp=7, out_data=None, in_fmt=F32)[0] == S.NULL
    # 4. interpolation, before the cameras (Lanczos-3 is refused)
    assert _compose(lrp, [bad_cam], (nan,), interp=7, n=0, in_fmt=F32)[0] == S.INTERPOLATION
    assert _compose(lrp, [good], interp=3)[0] == S.INTERPOLATION
    # 5. per camera, ascending, before the gains
    st, text = _compose(lrp, [good, bad_cam], (nan, nan), n=0, in_fmt=F32)
    assert st == S.BAD_ARG and "camera 1" in text and "model" in text
    st, text = _compose(lrp, [good, _with(good, data=None)], (nan, nan), n=0, in_fmt=F32)
    assert st == S.NULL and "camera 1" in text
    st, text = _compose(lrp, [good, _with(fish, fy=inf)], in_fmt=F32)
    assert st == S.BAD_ARG and "camera 1" in text and "fy" in text
    # the gains: after the cameras, before num_samples; the text names the camera
    for bad in (nan, inf, -inf, -1.0, -1e-30):
        st, text = _compose(lrp, [good, fish, good], (1.0, 1.0, bad), n=0, in_fmt=F32)
        assert st == S.BAD_ARG and "camera 2" in text and "gain" in text, bad
    # 6. num_samples, before the formats
    for n in (0, -1, 16):
        st, text = _compose(lrp, [good, fish], n=n, in_fmt=F32)
        assert st == S.BAD_ARG and "num_samples" in text
    # then formats and packed channel counts; float32 frames name the calls to make instead; in front of C > 8
    st, text = _compose(lrp, [good], in_fmt=F32, out_channels=9)
    assert st == S.BAD_ARG and "lrp_compose_cameras_device" in text and "lrp_compose_cameras_gain_device" in text and "lrp_encode_pixels_device" in text
    assert _compose(lrp, [good], in_fmt=3, out_channels=9)[0] == S.BAD_ARG and _compose(lrp, [good], in_fmt=-1)[0] == S.BAD_ARG
    assert _compose(lrp, [good], out_fmt=3, out_channels=9)[0] == S.BAD_ARG and _compose(lrp, [good], out_fmt=-1)[0] == S.BAD_ARG
    assert _compose(lrp, [good], in_pch=0, out_channels=9)[0] == S.BAD_ARG and _compose(lrp, [good], out_pch=0)[0] == S.BAD_ARG
    assert _compose(lrp, [good], in_pch=-4)[0] == S.BAD_ARG
    # more than 8 channels: in front of the size check of the packed frames
    big = _good(lrp, size=(1 << 14, 1 << 14))
    assert _compose(lrp, [_good(lrp, size=(1 << 13, 1 << 13))], out_channels=9, in_pch=64)[0] == S.CHANNELS  # (2^32 packed bytes)
    # every packed frame and the output fit 32-bit byte offsets: 2^31 bytes is the last size that does
    assert _compose(lrp, [big], out_channels=1, in_pch=8)[0] == S.NO_DEVICE
    assert _compose(lrp, [good, big], out_channels=1, in_pch=9)[0] == S.BAD_DIMS
    assert _compose(lrp, [big], out_channels=1, in_fmt=F16, in_pch=4)[0] == S.NO_DEVICE
    assert _compose(lrp, [big], out_channels=1, in_fmt=F16, in_pch=5)[0] == S.BAD_DIMS
    assert _compose(lrp, [good], out_channels=1, out_size=(1 << 14, 1 << 14), out_fmt=F32, out_pch=2)[0] == S.NO_DEVICE
    st, text = _compose(lrp, [good], out_channels=1, out_size=(1 << 14, 1 << 14), out_fmt=F32, out_pch=3)
    assert st == S.BAD_DIMS and "2^31 bytes" in text
    assert _compose(lrp, [big], out_channels=1, in_pch=(1 << 31) - 1)[0] == S.BAD_DIMS  # (no overflow in the product)


def test_overlap_argument_errors_in_the_documented_order(lrp):
    S, L = lrp.Status, lrp.LensInfo
    good, fish = _good(lrp), _good(lrp, 1)
    nan, inf = math.nan, math.inf
    bad_cam = _with(good, model=5)
    # good calls get as far as the device; out->data may be NULL; the ends of the range are allowed
    assert _overlap(lrp, [good, fish, good])[0] == S.NO_DEVICE and _overlap(lrp, [good] * 8, out_data=None, in_fmt=F16)[0] == S.NO_DEVICE
    assert _overlap(lrp, [good], lo=0.0, hi=32768.0, in_pch=1, out_channels=8)[0] == S.NO_DEVICE
    # the errors of lrp_camera_overlap_device, in its order, each in front of a packed-format error
    for k in (0, 9):
        st, text = _overlap(lrp, [good] * k, null_out=True, stats=None, lo=nan, in_fmt=F32)
        assert st == S.BAD_ARG and "n_in" in text
    assert _overlap(lrp, [good], null_cams=True, out_channels=0, in_fmt=F32)[0] == S.NULL
    assert _overlap(lrp, [good], null_out=True, stats=None, in_fmt=F32)[0] == S.NULL
    lrp.lens_extensions(0)
    assert _overlap(lrp, [bad_cam], lout=L.stereographic(10.0, 36.0, 8, 8), out_channels=0, in_fmt=F32)[0] == S.OUTPUT_LENS
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    assert _overlap(lrp, [bad_cam], out_channels=0, out_size=(0, 8), in_fmt=F32)[0] == S.CHANNELS
    assert _overlap(lrp, [bad_cam], out_size=(0, 8), in_fmt=F32)[0] == S.BAD_DIMS
    st, text = _overlap(lrp, [good, bad_cam, _with(good, width=0)], stats=None, lo=nan, out_data=None, in_fmt=F32)
    assert st == S.BAD_ARG and "camera 1" in text and "model" in text
    st, text = _overlap(lrp, [good, good, _with(good, data=None, fx=nan)], stats=None, in_fmt=F32)
    assert st == S.NULL and "camera 2" in text
    st, text = _overlap(lrp, [good], stats=None, lo=nan, in_fmt=F32)
    assert st == S.NULL and "stats" in text
    for lo, hi in ((nan, 0.5), (0.1, nan), (-1e-9, 0.5), (0.6, 0.5), (0.5, 32768.5)):
        st, text = _overlap(lrp, [good, fish], lo=lo, hi=hi, in_fmt=F32)
        assert st == S.BAD_ARG and "lo" in text, (lo, hi)
    # then the packed errors
    st, text = _overlap(lrp, [good], in_fmt=F32, out_channels=9)
    assert st == S.BAD_ARG and "lrp_camera_overlap_device" in text
    assert _overlap(lrp, [good], in_fmt=3, out_channels=9)[0] == S.BAD_ARG and _overlap(lrp, [good], in_fmt=-1)[0] == S.BAD_ARG
    assert _overlap(lrp, [good], in_pch=0, out_channels=9)[0] == S.BAD_ARG
    assert _overlap(lrp, [_good(lrp, size=(1 << 13, 1 << 13))], out_channels=9, in_pch=64)[0] == S.CHANNELS
    big = _good(lrp, size=(1 << 14, 1 << 14))
    assert _overlap(lrp, [big], out_channels=1, in_pch=8)[0] == S.NO_DEVICE and _overlap(lrp, [good, big], out_channels=1, in_pch=9)[0] == S.BAD_DIMS
    assert _overlap(lrp, [big], out_channels=1, in_fmt=F16, in_pch=5)[0] == S.BAD_DIMS
    # (there is no packed output: a target of any size the parent accepts)
    assert _overlap(lrp, [good], out_channels=1, out_size=(1 << 15, 1 << 15), out_data=None)[0] == S.NO_DEVICE


def test_python_mirrors_refuse_before_the_library(lrp):
    import torch

    sc = kp.rig_scene(lrp)
    s = kp.FORMATS["rgba8"]
    cams, out = kp.cameras(lrp, sc), kp.out_image(lrp, s, sc)
    host_np = [np.zeros((c["size"][1], c["size"][0], 4), np.uint8) for c in sc["cams"]]
    host_t = [torch.from_numpy(a) for a in host_np]
    out_t = torch.zeros((48, 80, 4), dtype=torch.uint8)
    for datas in (host_np, host_t, host_t[:2] + host_np[2:]):
        with pytest.raises(ValueError, match="device tensors only"):
            lrp.compose_cameras_packed(cams, U8, datas, out, U8, out_t, 255, 2, 2)
        with pytest.raises(ValueError, match="device tensors only"):
            lrp.camera_overlap_packed(cams, U8, datas, out)
    with pytest.raises(ValueError, match="3 cameras but 1 packed tensors"):
        lrp.compose_cameras_packed(cams, U8, host_t[:1], out, U8, out_t, 255, 2, 2)
    with pytest.raises(ValueError, match="3 cameras but 2 packed tensors"):
        lrp.camera_overlap_packed(cams, U8, host_t[:2], out)


class _FakeCuda:
    """What the mirrors ask of a tensor, without a device: for the checks that come after `is_cuda`."""

    is_cuda = True

    def __init__(self, shape, itemsize, dtype="fake"):
        self.shape, self._itemsize, self.dtype = tuple(shape), itemsize, dtype

    def is_contiguous(self):
        return True

    def element_size(self):
        return self._itemsize

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def data_ptr(self):
        raise AssertionError("a pointer was taken before the checks were done")


def test_python_mirrors_check_every_tensor(lrp, monkeypatch):
    """Element size against the format, numel against the camera, one packed channel count, the output, the planes, the gains and
    the stats tensor — for every camera, not the first alone; no data_ptr() is taken before."""
    monkeypatch.setattr(lrp, "_is_torch", lambda t: isinstance(t, _FakeCuda) or type(t).__module__.startswith("torch"))
    import torch

    sc = kp.rig_scene(lrp)
    s = kp.FORMATS["rgba8"]
    cams, out = kp.cameras(lrp, sc), kp.out_image(lrp, s, sc)
    good = [_FakeCuda((c["size"][1], c["size"][0], 4), 1) for c in sc["cams"]]
    good_out = _FakeCuda((48, 80, 4), 1)

    def both(datas, fmt, match):
        with pytest.raises(ValueError, match=match):
            lrp.compose_cameras_packed(cams, fmt, datas, out, U8, good_out, 0, 2, 2)
        with pytest.raises(ValueError, match=match):
            lrp.camera_overlap_packed(cams, fmt, datas, out)

    both(good[:2] + [_FakeCuda((48, 64, 4), 2)], U8, r"in_datas\[2\]: elements of 2 bytes")
    both(good, F16, r"in_datas\[0\]: elements of 1 bytes")
    both(good[:1] + [_FakeCuda((40, 55, 4), 1)] + good[2:], U8, r"in_datas\[1\]: packed tensors must hold")
    both(good[:2] + [_FakeCuda((48, 64, 3), 1)], U8, "same number of packed channels")
    with pytest.raises(ValueError, match="out_data: elements of 1 bytes"):
        lrp.compose_cameras_packed(cams, U8, good, out, F32, good_out, 0, 2, 2)
    with pytest.raises(ValueError, match="out_data: packed tensors must hold"):
        lrp.compose_cameras_packed(cams, U8, good, out, U8, _FakeCuda((48, 79, 4), 1), 0, 2, 2)
    with pytest.raises(ValueError, match="out_data must be a contiguous CUDA tensor"):
        lrp.compose_cameras_packed(cams, U8, good, out, U8, np.zeros((48, 80, 4), np.uint8), 0, 2, 2)
    bad_planes = (torch.zeros((48, 80), dtype=torch.float32), torch.zeros((48, 79), dtype=torch.uint8), torch.zeros((48, 80), dtype=torch.uint8),
                  np.zeros((48, 80), dtype=np.uint8))  # (the last two: not device tensors)
    for bad in bad_planes:
        with pytest.raises(ValueError, match="count must be"):
            lrp.compose_cameras_packed(cams, U8, good, out, U8, good_out, 0, 2, 2, count=bad)
        with pytest.raises(ValueError, match="coverage must be"):
            lrp.compose_cameras_packed(cams, U8, good, out, U8, good_out, 0, 2, 2, coverage=bad)
    with pytest.raises(ValueError, match="one value per camera"):
        lrp.compose_cameras_packed(cams, U8, good, out, U8, good_out, 0, 2, 2, gains=(1.0, 1.0))
    for bad in (torch.zeros((8, 8, 2), dtype=torch.int64), np.zeros((8, 8, 2), dtype=np.int64)):  # not device tensors
        with pytest.raises(ValueError, match="stats must be"):
            lrp.camera_overlap_packed(cams, U8, good, out, stats=bad)


# ------------------------------------------------------------------ every case discriminates
def _check(lrp, s, sc, gains, n, interp, mode, what, stats=None, packed=None):
    packed = packed if packed is not None else kp.make_inputs(s, sc)
    out, count, m = kp.cpu_chain(lrp, s, sc, packed, gains, n, interp, mode)
    ow, oh = sc["size"]
    assert out.shape == (oh, ow, s["out_pch"]) and out.dtype == kp.pc.NUMPY_TYPES[s["out_fmt"]] and count.shape == m.shape == (oh, ow)
    why = kp.discriminates(s, out, count, m, n)
    assert why is None, f"{what}: {why}"
    copy = min(s["C"], s["out_pch"])
    assert (kp.pc.as_bytes(out[..., :copy][m == 0]) == 0).all(), f"{what}: an m == 0 pixel encodes +0.0f"
    if copy < s["out_pch"]:
        mask = {U8: 0xFF, F16: 0xFFFF, F32: 0xFFFFFFFF}[s["out_fmt"]]
        tail = np.ascontiguousarray(out[..., copy:]).view(np.uint32) if s["out_fmt"] == F32 else out[..., copy:]
        assert (tail == (s["fill"] & mask)).all(), f"{what}: the fill behind C"
    return out, count, m


@pytest.mark.parametrize("fmt", list(kp.FORMATS))
@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_rig_cases_discriminate(lrp, out_name, fmt):
    """The rig in front of the five target lenses: 3 samplers x 3 modes at n = 1, with GAINS at n = 2."""
    s, sc = kp.FORMATS[fmt], kp.rig_scene(lrp, out_name)
    packed = kp.make_inputs(s, sc)
    for interp in (0, 1, 2):
        for mode in kp.MODES:
            _check(lrp, s, sc, None, 1, interp, mode, f"{out_name} {fmt} interp {interp} mode {mode}", packed=packed)
            _check(lrp, s, sc, kp.GAINS, 2, interp, mode, f"{out_name} {fmt} gains interp {interp} mode {mode}", packed=packed)


@pytest.mark.parametrize("n", [2, 15])
def test_rig_n_cases_discriminate(lrp, n):
    for out_name in ("eqr_part", "rect18"):
        for fmt in kp.FORMATS:
            _check(lrp, kp.FORMATS[fmt], kp.rig_scene(lrp, out_name), None, n, 1, kp.MEAN, f"{out_name} {fmt} n {n}")


@pytest.mark.parametrize("name", list(kp.CHANNEL_SETUPS))
def test_channel_setups_discriminate(lrp, name):
    s, sc = kp.CHANNEL_SETUPS[name], kp.rig_scene(lrp)
    for n, interp, mode in ((1, 2, kp.FEATHER), (2, 1, kp.MEAN), (2, 0, kp.FIRST)):
        _check(lrp, s, sc, kp.GAINS, n, interp, mode, f"{name} n {n} interp {interp} mode {mode}")


def test_eight_cameras_discriminate(lrp):
    for fmt in kp.FORMATS:
        _check(lrp, kp.FORMATS[fmt], kp.eight_scene(lrp), None, 2, 2, kp.FEATHER, f"eight {fmt}")


def test_overlap_cases_discriminate(lrp):
    """Under RANGE on decoded 8-bit noise: three pairs with N_ij > 0, and the range excludes at least a quarter of what both
    cameras cover (the table under lo = 0, hi = 32768, where every decoded 8-bit luminance is valid)."""
    s = kp.FORMATS["rgba8"]
    for out_name in cam.OUT_LENSES:
        sc = kp.rig_scene(lrp, out_name)
        packed = kp.make_inputs(s, sc)
        got = kp.cpu_overlap(lrp, s, sc, packed, *kp.RANGE)
        both = kp.cpu_overlap(lrp, s, sc, packed, 0.0, 32768.0)
        for i, j in ((0, 1), (0, 2), (1, 2)):
            print(f"{out_name}: pair {i}{j} N {got[i, j, 0]} of {both[i, j, 0]}")
            assert got[i, j, 0] > 0 and got[i, j, 0] * 4 <= both[i, j, 0] * 3, (out_name, i, j, got[i, j, 0], both[i, j, 0])
        assert (got[3:] == 0).all() and (got[:, 3:] == 0).all()
