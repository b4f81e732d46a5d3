"""CPU: lrp_compose_cameras_multiband_packed_device (include/lrp.h "multi-band blending, packed pixels") without a device — the
symbol and its Python mirror exist, the argument errors come in the documented order with the documented statuses (all of them
before a device is touched; valid arguments get as far as LRP_ERR_NO_DEVICE; every item of the float call wins over every packed
item), the mirror refuses what it must before any pointer reaches the library, and every case of tests/multiband_packed_cases.py
discriminates on the chain on the CPU (cpu_chain: numpy decode -> the model of tests/multiband_model.py -> numpy encode):
  - `label` takes at least two camera values, and 255 where the scene has uncovered pixels;
  - at least one seam pixel exists;
  - for an 8-bit output at least half of the covered pixels carry a colour code in 1 .. 254, and at least 32 distinct codes occur.
The 1 x 1 target has one label, no pair of neighbours and 3 colour samples; it alone is held to a covered pixel.  The planted
specials show in every case of their group: the model's NaN samples are NaNs (code 255) in the output, finite ones are not all."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest

import camera_cases as cam
import camera_packed_cases as kp
import multiband_packed_cases as mp

F32, F16, U8 = mp.F32, mp.F16, mp.U8
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


def _call(lrp, cams, gains=None, in_fmt=U8, in_pch=4, out_fmt=U8, out_pch=4, interp=2, bands=3, scratch=0x100000, scratch_bytes=1 << 40,
          null_cams=False, null_out=False, lout=None, out_channels=4, out_size=(8, 8), out_data=0x2000):
    lib = lrp._native.load()
    k = len(cams)
    arr = (lrp._native.LrpCamera * max(k, 1))(*cams)
    cout = lrp.Image(lout or lrp.LensInfo.equirectangular(), out_size[0], out_size[1], out_channels, None).to_c()
    cout.data = out_data
    g = None if gains is None else np.asarray(gains, dtype=np.float32)
    st = lib.lrp_compose_cameras_multiband_packed_device(None if null_cams else arr, k, in_fmt, in_pch, None, None if g is None else g.ctypes.data,
                                                         None if null_out else ctypes.byref(cout), out_fmt, out_pch, 255, interp, bands, None, None,
                                                         None, scratch, scratch_bytes, -1, None)
    return st, lib.lrp_last_error().decode()


def test_symbol_and_python_mirror_exist(lrp):
    lib = lrp._native.load()
    name = "lrp_compose_cameras_multiband_packed_device"
    assert hasattr(lib, name) and name in lrp._native.SYMBOLS
    assert lib.lrp_abi_version() == 3
    with open(os.path.join(ROOT, "include", "lrp.h")) as f:
        header = f.read()
    assert "int lrp_compose_cameras_multiband_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels," in header
    assert "#define LRP_ABI_VERSION 3" in header
    sig = inspect.signature(lrp.compose_cameras_multiband_packed).parameters
    assert list(sig) == ["cameras", "in_format", "in_datas", "out_image", "out_format", "out_data", "out_fill", "interpolation",
                         "rotation_matrices", "num_bands", "gains", "post", "count", "label", "scratch", "device", "stream"]
    assert sig["num_bands"].default == 5 and all(sig[n].default is None for n in list(sig)[8:] if n != "num_bands")


def test_argument_errors_in_the_documented_order(lrp):
    S, L = lrp.Status, lrp.LensInfo
    good, fish = _good(lrp), _good(lrp, 1)
    nan = math.nan
    bad_cam = _with(good, model=5)
    need = lrp.multiband_scratch_bytes(8, 8, 4, 3)
    # valid arguments reach the device: both source formats, every output format, every sampler, every band count, every C
    for in_fmt in (F16, U8):
        for out_fmt in (F32, F16, U8):
            for interp in (0, 1, 2):
                assert _call(lrp, [good, fish], in_fmt=in_fmt, out_fmt=out_fmt, interp=interp)[0] == S.NO_DEVICE
    for bands in range(9):
        assert _call(lrp, [good, fish, good], bands=bands)[0] == S.NO_DEVICE
    for channels in (1, 2, 3, 4):
        assert _call(lrp, [good], out_channels=channels, in_pch=7, out_pch=64)[0] == S.NO_DEVICE
    assert _call(lrp, [good] * 8, gains=[0.0] * 8, scratch_bytes=need)[0] == S.NO_DEVICE
    # the named refusals, each alone
    assert _call(lrp, [good], in_fmt=F32)[0] == S.BAD_ARG and _call(lrp, [good], in_fmt=7)[0] == S.BAD_ARG
    assert _call(lrp, [good], out_fmt=7)[0] == S.BAD_ARG
    assert _call(lrp, [good], in_pch=0)[0] == S.BAD_ARG and _call(lrp, [good], out_pch=0)[0] == S.BAD_ARG
    assert _call(lrp, [good], out_channels=5)[0] == S.CHANNELS
    st, text = _call(lrp, [good], bands=9)
    assert st == S.BAD_ARG and "num_bands" in text

    # items 1 to 6 of the float call, in its order — each wins over each packed item
    packed_items = (dict(in_fmt=F32), dict(in_fmt=7), dict(out_fmt=7), dict(in_pch=0), dict(out_pch=0), dict(in_pch=(1 << 31) - 1),
                    dict(out_fmt=F32, out_pch=(1 << 31) - 1))

    def float_item(cams, status, word=None, **kw):
        for packed in (dict(),) + packed_items:
            st, text = _call(lrp, cams, **kw, **packed)
            assert st == status and (word is None or word in text), (kw, packed, st, text)

    # 1. n_in; NULL; the output side; the interpolation; the cameras; the gains
    for k in (0, 9):
        float_item([good] * k, S.BAD_ARG, "n_in", null_out=True, interp=7, bands=9, scratch=None)
    float_item([good], S.NULL, null_cams=True, interp=7, bands=9)
    float_item([good], S.NULL, null_out=True, bands=9)
    lrp.lens_extensions(0)
    float_item([bad_cam], S.OUTPUT_LENS, lout=L.stereographic(10.0, 36.0, 8, 8), interp=7, out_channels=0)
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    float_item([bad_cam], S.CHANNELS, interp=7, out_channels=0, out_size=(0, 8))
    float_item([bad_cam], S.BAD_DIMS, interp=7, out_size=(0, 8), out_data=None, out_channels=5)
    float_item([bad_cam], S.NULL, interp=7, out_data=None, out_channels=5)
    float_item([bad_cam], S.INTERPOLATION, gains=[nan], interp=7, out_channels=5)
    float_item([bad_cam], S.INTERPOLATION, gains=[nan], interp=3, out_channels=5)  # (Lanczos-3 is out of scope)
    float_item([good, bad_cam], S.BAD_ARG, "camera 1", gains=[nan, nan], out_channels=5, bands=9)
    float_item([good, _with(good, data=None)], S.NULL, "camera 1", gains=[nan, nan], out_channels=5)
    for bad in (nan, math.inf, -1.0):
        float_item([good, fish, good], S.BAD_ARG, "gain", gains=[1.0, 1.0, bad], out_channels=5, bands=9, scratch=None)
    # 2. more than 4 channels, before the bands
    float_item([good], S.CHANNELS, out_channels=5, bands=9, scratch=None)
    # 3. the bands, before the scratch
    for bands in (-1, 9):
        float_item([good], S.BAD_ARG, "num_bands", bands=bands, scratch=None)
    # 4. scratch NULL, before its size
    float_item([good], S.NULL, "scratch", scratch=None, scratch_bytes=0)
    # 5. alignment and size: the text states both sizes
    for scratch, size in ((0x100000 + 128, need), (0x100000, need - 1), (0x100000, 0)):
        float_item([good], S.BAD_ARG, str(need), scratch=scratch, scratch_bytes=size)
    # 6. a target taller than a launch grid of 8-row tiles, last of the float call's
    assert _call(lrp, [good], out_size=(1, 8 * 65535), out_channels=1)[0] == S.NO_DEVICE
    float_item([good], S.BAD_DIMS, "height", out_size=(1, 8 * 65535 + 1), out_channels=1)

    # then the packed items, in the order of lrp_compose_cameras_packed_device
    big = _good(lrp, size=(1 << 14, 1 << 14))
    st, text = _call(lrp, [good, big], in_fmt=F32, out_fmt=7, in_pch=0, out_pch=0)
    assert st == S.BAD_ARG and "lrp_compose_cameras_multiband_device" in text and "lrp_encode_pixels_device" in text
    for fmts in (dict(in_fmt=3), dict(in_fmt=-1), dict(out_fmt=3), dict(out_fmt=7)):
        st, text = _call(lrp, [good, big], in_pch=0, **fmts)
        assert st == S.BAD_ARG and "format" in text
    for pch in (dict(in_pch=0), dict(in_pch=-4), dict(out_pch=0)):
        st, text = _call(lrp, [good, big], **{**dict(in_pch=9), **pch})
        assert st == S.BAD_ARG and "packed channel counts" in text
    # every packed frame and the output fit 32-bit byte offsets: 2^31 bytes is the last size that does
    assert _call(lrp, [big], out_channels=1, in_pch=8)[0] == S.NO_DEVICE
    assert _call(lrp, [good, big], out_channels=1, in_pch=9)[0] == S.BAD_DIMS
    assert _call(lrp, [big], out_channels=1, in_fmt=F16, in_pch=4)[0] == S.NO_DEVICE
    assert _call(lrp, [big], out_channels=1, in_fmt=F16, in_pch=5)[0] == S.BAD_DIMS
    assert _call(lrp, [good], out_channels=1, out_size=(1 << 14, 1 << 14), out_fmt=F32, out_pch=2)[0] == S.NO_DEVICE
    st, text = _call(lrp, [good], out_channels=1, out_size=(1 << 14, 1 << 14), out_fmt=F32, out_pch=3)
    assert st == S.BAD_DIMS and "2^31 bytes" in text
    assert _call(lrp, [big], out_channels=1, in_pch=(1 << 31) - 1)[0] == S.BAD_DIMS  # (no overflow in the product)
    # last, this call's own: a camera's float32 level-0 layer, W x H x C x 4 bytes, fits 32-bit byte offsets too — it is up to four
    # times the packed output, which passes the item above in every call here
    assert _call(lrp, [good], out_channels=4, out_size=(1 << 14, 1 << 13))[0] == S.NO_DEVICE  # 2^31 bytes: the last size that does
    for kw in (dict(out_channels=4, out_size=(1 << 14, (1 << 13) + 1)), dict(out_channels=4, out_size=(1 << 15, 1 << 14)),  # (RGBA8 of 2^31 bytes)
               dict(out_channels=3, out_size=(1 << 14, 1 << 14), out_pch=3), dict(out_channels=2, out_size=(1 << 14, (1 << 14) + 1), out_fmt=F16, out_pch=2)):
        st, text = _call(lrp, [good], **kw)
        assert st == S.BAD_DIMS and "level-0 layer" in text, (kw, st, text)
    assert _call(lrp, [good], out_channels=1, out_size=(1 << 15, 1 << 14), out_pch=1)[0] == S.NO_DEVICE
    st, text = _call(lrp, [good], out_channels=1, out_size=(1 << 15, (1 << 14) + 1), out_pch=1)
    assert st == S.BAD_DIMS and "level-0 layer" in text
    # ... behind every other item: the float call's (the scratch) and the packed ones
    assert _call(lrp, [good], out_channels=4, out_size=(1 << 15, 1 << 14), scratch_bytes=0)[0] == S.BAD_ARG
    st, text = _call(lrp, [good], out_channels=4, out_size=(1 << 15, 1 << 14), in_fmt=F32)
    assert st == S.BAD_ARG and "lrp_encode_pixels_device" in text
    st, text = _call(lrp, [good], out_channels=4, out_size=(1 << 15, 1 << 14), out_pch=5)
    assert st == S.BAD_DIMS and "2^31 bytes cannot be addressed" in text


def test_python_mirror_refuses_before_the_library(lrp):
    import torch

    sc = kp.rig_scene(lrp)
    s = mp.FORMATS["rgba8"]
    cams, out = kp.cameras(lrp, sc), kp.out_image(lrp, s, sc)
    host_np = [np.zeros((c["size"][1], c["size"][0], 4), np.uint8) for c in sc["cams"]]
    host_t = [torch.from_numpy(a) for a in host_np]
    out_t = torch.zeros((48, 80, 4), dtype=torch.uint8)
    for datas in (host_np, host_t, host_t[:2] + host_np[2:]):
        with pytest.raises(ValueError, match="device tensors only"):
            lrp.compose_cameras_multiband_packed(cams, U8, datas, out, U8, out_t, 255, 2)
    with pytest.raises(ValueError, match="3 cameras but 1 packed tensors"):
        lrp.compose_cameras_multiband_packed(cams, U8, host_t[:1], out, U8, out_t, 255, 2)


class _FakeCuda:
    """What the mirror asks of a tensor, without a device: for the checks that come after `is_cuda`."""

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


def test_python_mirror_checks_every_tensor(lrp, monkeypatch):
    """Element size against the format, numel against the camera, one packed channel count, the output, the planes, the gains and
    the scratch — for every camera, not the first alone; no data_ptr() is taken before."""
    monkeypatch.setattr(lrp, "_is_torch", lambda t: isinstance(t, _FakeCuda) or type(t).__module__.startswith("torch"))
    import torch

    sc = kp.rig_scene(lrp)
    s = mp.FORMATS["rgba8"]
    cams, out = kp.cameras(lrp, sc), kp.out_image(lrp, s, sc)
    good = [_FakeCuda((c["size"][1], c["size"][0], 4), 1) for c in sc["cams"]]
    good_out = _FakeCuda((48, 80, 4), 1)

    def refused(match, datas=good, fmt=U8, out_fmt=U8, out_data=good_out, **kw):
        with pytest.raises(ValueError, match=match):
            lrp.compose_cameras_multiband_packed(cams, fmt, datas, out, out_fmt, out_data, 0, 2, device=0, **kw)

    refused(r"in_datas\[2\]: elements of 2 bytes", good[:2] + [_FakeCuda((48, 64, 4), 2)])
    refused(r"in_datas\[0\]: elements of 1 bytes", fmt=F16)
    refused(r"in_datas\[1\]: packed tensors must hold", good[:1] + [_FakeCuda((40, 55, 4), 1)] + good[2:])
    refused("same number of packed channels", good[:2] + [_FakeCuda((48, 64, 3), 1)])
    refused("out_data: elements of 1 bytes", out_fmt=F32)
    refused("out_data: packed tensors must hold", out_data=_FakeCuda((48, 79, 4), 1))
    refused("out_data must be a contiguous CUDA tensor", out_data=np.zeros((48, 80, 4), np.uint8))
    bad_planes = (torch.zeros((48, 80), dtype=torch.float32), torch.zeros((48, 79), dtype=torch.uint8), torch.zeros((48, 80), dtype=torch.uint8),
                  np.zeros((48, 80), dtype=np.uint8))  # (the last two: not device tensors)
    for bad in bad_planes:
        refused("count must be", count=bad)
        refused("label must be", label=bad)
    refused("one value per camera", gains=(1.0, 1.0))
    for bad in (torch.zeros((1 << 20,), dtype=torch.uint8), np.zeros((1 << 20,), dtype=np.uint8), _FakeCuda((1 << 20,), 4, torch.float32)):
        refused("scratch must be a contiguous uint8 CUDA tensor", scratch=bad)


# ------------------------------------------------------------------ every case discriminates
@pytest.mark.parametrize("group", sorted({c["group"] for c in mp.CASES}))
def test_cases_discriminate(lrp, group):
    seen = {}
    for c in mp.group(group):
        s, sc = c["s"], c["scene"](lrp)
        img, count, label = mp.cpu_float(lrp, s, sc, c["inputs"](s, sc), c["gains"], c["interp"], c["bands"])
        out = mp.pc.encode_numpy(lrp, img, s["out_fmt"], s["out_pch"], s["fill"])
        ow, oh = sc["size"]
        if group == "specials":
            why = mp.nan_reaches(s, out, img)
            assert why is None, f"{c['name']}: {why}"
        assert out.shape == (oh, ow, s["out_pch"]) and out.dtype == mp.pc.NUMPY_TYPES[s["out_fmt"]] and count.shape == label.shape == (oh, ow)
        if c["full"]:
            why = mp.discriminates(s, out, count, label, c["uncovered"], c["cameras"])
            assert why is None, f"{c['name']}: {why}"
        else:
            assert (label != mp.NO_CAMERA).any(), f"{c['name']}: no covered pixel"
        copy = min(s["C"], s["out_pch"])
        assert (mp.pc.as_bytes(out[..., :copy][label == mp.NO_CAMERA]) == 0).all(), f"{c['name']}: an uncovered pixel encodes +0.0f"
        if copy < s["out_pch"]:
            mask = {U8: 0xFF, F16: 0xFFFF, F32: 0xFFFFFFFF}[s["out_fmt"]]
            tail = np.ascontiguousarray(out[..., copy:]).view(np.uint32) if s["out_fmt"] == F32 else out[..., copy:]
            assert (tail == (s["fill"] & mask)).all(), f"{c['name']}: the fill behind C"
        seen[c["name"]] = out
    assert len(seen) == len(mp.group(group)), "case names repeat"
    if group == "specials":  # an infinity reaches the output too (through three bands one meets another: B == 0 keeps them)
        assert ((seen["half-B0-interp0-plain"] & 0x7FFF) == 0x7C00).any()


def test_groups_compare_one_case_each_against_the_cpu_chain():
    for group in {c["group"] for c in mp.CASES}:
        assert any(c["cpu"] for c in mp.group(group)), group
