"""CPU: lrp_compose_packed_device (include/lrp.h "compose, packed pixels") without a device — the symbol and its Python mirror
exist, the argument errors come in the documented order with the documented statuses (all of them before a device is touched;
valid arguments get as far as LRP_ERR_NO_DEVICE), the Python mirror refuses what it must before any pointer reaches the
library, and every case of tests/compose_packed_cases.py discriminates: among the samples of the pixels with k >= 1 of the
chain on the CPU there are at least 64 distinct codes and no code makes up more than a quarter.  (The k == 0 pixels are one
code by definition and may be 71 % of an output: the condition is on the covered pixels.)"""
import ctypes
import inspect
import os

import numpy as np
import pytest

import compose_cases as cs
import compose_packed_cases as cp
import coverage_cases as cc

F32, F16, U8 = cp.F32, cp.F16, cp.U8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def extensions_on(lrp):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    try:
        yield
    finally:
        lrp.lens_extensions(prev)


def _status(lrp, lenses, lout=None, in_fmt=U8, in_pch=4, out_fmt=U8, out_pch=4, mode=0, interp=2, channels=None, out_channels=4, in_size=(8, 8),
            out_size=(8, 8), rotations=False, null=None):
    lib = lrp._native.load()
    n = len(lenses)
    lout = lout or lrp.LensInfo.equirectangular()
    channels = channels or [out_channels] * n
    arr = (lrp._native.LrpImage * max(n, 1))()
    for i, lin in enumerate(lenses):
        arr[i] = lrp.Image(lin, in_size[0], in_size[1], channels[i], None).to_c()
        arr[i].data = None if null == f"data{i}" else 0x1000  # never dereferenced: every call here fails, in validation or at device -1
    cout = lrp.Image(lout, out_size[0], out_size[1], out_channels, None).to_c()
    cout.data = None if null == "out_data" else 0x2000
    rot = np.tile(np.eye(3, dtype=np.float32).reshape(9), max(n, 1)) if rotations else None
    st = lib.lrp_compose_packed_device(None if null == "ins" else arr, n, in_fmt, in_pch, rot.ctypes.data if rotations else None,
                                       None if null == "out" else ctypes.byref(cout), out_fmt, out_pch, 255, interp, mode, None, None, -1, None)
    return st, lib.lrp_last_error().decode()


def test_symbol_and_python_mirror_exist(lrp):
    lib = lrp._native.load()
    assert hasattr(lib, "lrp_compose_packed_device") and "lrp_compose_packed_device" in lrp._native.SYMBOLS
    assert lib.lrp_abi_version() == 3
    with open(os.path.join(ROOT, "include", "lrp.h")) as f:
        assert "int lrp_compose_packed_device(const lrp_image *ins, int n_in, int in_format, int in_packed_channels," in f.read()
    names = list(inspect.signature(lrp.compose_packed).parameters)
    assert names == ["in_images", "in_format", "in_datas", "out_image", "out_format", "out_data", "out_fill", "interpolation", "rotation_matrices",
                     "mode", "post", "count", "device", "stream"]


def test_argument_errors_in_the_documented_order(lrp):
    S, L = lrp.Status, lrp.LensInfo
    rect, pano, fish = L.rectilinear(18.0, 36.0, 8, 8), L.equirectangular(), L.equidistant(3.0)
    # 1. the errors of lrp_compose_device, in its order — each of them wins over a packed-format error (in_fmt F32 / 9, in_pch 0)
    assert _status(lrp, [], in_fmt=F32)[0] == S.BAD_ARG and "n_in" in _status(lrp, [], in_fmt=F32)[1]
    assert _status(lrp, [rect] * 9, in_fmt=9)[0] == S.BAD_ARG and "n_in" in _status(lrp, [rect] * 9, in_fmt=9)[1]
    st, text = _status(lrp, [rect] * 2, mode=3, in_fmt=F32)
    assert st == S.BAD_ARG and "mode" in text and _status(lrp, [rect], mode=-1)[0] == S.BAD_ARG
    assert _status(lrp, [rect], null="ins", in_fmt=F32)[0] == S.NULL and _status(lrp, [rect], null="out", in_pch=0)[0] == S.NULL
    assert _status(lrp, [rect] * 2, interp=3, in_fmt=F32)[0] == S.INTERPOLATION  # (Lanczos-3 is refused, bit on or off)
    assert _status(lrp, [rect, rect], channels=[4, 3], in_fmt=F32)[0] == S.CHANNELS
    assert _status(lrp, [rect, rect], channels=[3, 3], out_channels=4, in_fmt=9)[0] == S.CHANNELS
    assert _status(lrp, [rect], in_size=(0, 8), in_fmt=9)[0] == S.BAD_DIMS and _status(lrp, [rect], out_size=(8, -1), in_pch=0)[0] == S.BAD_DIMS
    assert _status(lrp, [rect], in_size=(1 << 15, 1 << 15), in_fmt=9)[0] == S.BAD_DIMS  # 2^32 floats
    assert _status(lrp, [rect, rect], null="data1", in_fmt=F32)[0] == S.NULL and _status(lrp, [rect], null="out_data", out_pch=0)[0] == S.NULL
    st, text = _status(lrp, [rect, fish], in_fmt=F32)  # the mode mix: the last of the compose errors, still in front of the format
    assert st == S.BAD_ARG and "rectilinear" in text and "equidistant" in text
    st, text = _status(lrp, [pano, L.equirectangular(-1.0, 1.0, -0.5, 0.5)], lout=rect, in_pch=0)
    assert st == S.BAD_ARG and "wrapping equirectangular" in text and "clamped equirectangular" in text
    # 2. formats and packed channel counts; float32 sources name the two calls to make instead; in front of C > 8
    st, text = _status(lrp, [rect], in_fmt=F32, out_channels=9)
    assert st == S.BAD_ARG and "lrp_compose_device" in text and "lrp_encode_pixels_device" in text
    assert _status(lrp, [rect], in_fmt=3, out_channels=9)[0] == S.BAD_ARG and _status(lrp, [rect], in_fmt=-1)[0] == S.BAD_ARG
    assert _status(lrp, [rect], out_fmt=3, out_channels=9)[0] == S.BAD_ARG and _status(lrp, [rect], out_fmt=-1)[0] == S.BAD_ARG
    assert _status(lrp, [rect], in_pch=0, out_channels=9)[0] == S.BAD_ARG and _status(lrp, [rect], out_pch=0)[0] == S.BAD_ARG
    assert _status(lrp, [rect], in_pch=-4)[0] == S.BAD_ARG
    # 3. more than 8 channels: in front of the size check of the packed images
    assert _status(lrp, [rect], out_channels=9, in_size=(1 << 13, 1 << 13), in_pch=64)[0] == S.CHANNELS  # (2^32 packed bytes)
    assert _status(lrp, [rect] * 2, out_channels=8, in_fmt=F16, in_pch=8, out_pch=8)[0] == S.NO_DEVICE
    # 4. every packed image fits 32-bit byte offsets: 2^31 bytes is the last size that does
    big = (1 << 14, 1 << 14)
    assert _status(lrp, [rect], out_channels=1, in_size=big, in_pch=8)[0] == S.NO_DEVICE  # 2^31 bytes of 8-bit samples
    assert _status(lrp, [rect], out_channels=1, in_size=big, in_pch=9)[0] == S.BAD_DIMS
    assert _status(lrp, [rect], out_channels=1, in_size=big, in_fmt=F16, in_pch=4)[0] == S.NO_DEVICE
    assert _status(lrp, [rect], out_channels=1, in_size=big, in_fmt=F16, in_pch=5)[0] == S.BAD_DIMS
    assert _status(lrp, [rect], out_channels=1, out_size=big, out_fmt=F32, out_pch=2)[0] == S.NO_DEVICE
    st, text = _status(lrp, [rect], out_channels=1, out_size=big, out_fmt=F32, out_pch=3)
    assert st == S.BAD_DIMS and "2^31 bytes" in text
    assert _status(lrp, [rect], out_channels=1, in_size=big, in_pch=(1 << 31) - 1)[0] == S.BAD_DIMS  # (no overflow in the product)
    # valid arguments reach the device: both source formats, every output format, every sampler and mode, 1 and 8 sources
    for in_fmt in (F16, U8):
        for out_fmt in (F32, F16, U8):
            for interp in (0, 1, 2):
                assert _status(lrp, [rect, rect], in_fmt=in_fmt, out_fmt=out_fmt, interp=interp, mode=interp)[0] == S.NO_DEVICE
    assert _status(lrp, [rect] * 8, rotations=True)[0] == S.NO_DEVICE and _status(lrp, [fish], out_channels=1, in_pch=7, out_pch=64)[0] == S.NO_DEVICE


def test_extension_lenses_need_their_bit(lrp):
    S, L = lrp.Status, lrp.LensInfo
    rect, pano = L.rectilinear(18.0, 36.0, 8, 8), L.equirectangular()
    eqs, stg = L.equisolid(10.0, 36.0, 3.0, 8, 8), L.stereographic(10.0, 36.0, 8, 8)
    assert _status(lrp, [eqs, eqs])[0] == S.NO_DEVICE and _status(lrp, [stg], lout=stg)[0] == S.NO_DEVICE
    lrp.lens_extensions(lrp.LENS_EXT_STEREOGRAPHIC)
    assert _status(lrp, [eqs, eqs], in_fmt=F32)[0] == S.INPUT_LENS and _status(lrp, [rect], lout=eqs, in_fmt=F32)[0] == S.OUTPUT_LENS
    assert _status(lrp, [rect, eqs])[0] == S.INPUT_LENS  # (the second source's lens check comes before the mode mix)
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID)
    assert _status(lrp, [stg, stg])[0] == S.INPUT_LENS and _status(lrp, [rect], lout=stg)[0] == S.OUTPUT_LENS
    lrp.lens_extensions(0)
    assert _status(lrp, [eqs])[0] == S.INPUT_LENS and _status(lrp, [stg])[0] == S.INPUT_LENS


def test_python_mirror_refuses_before_the_library(lrp):
    import torch

    rect, pano = lrp.LensInfo.rectilinear(18.0, 36.0, 8, 8), lrp.LensInfo.equirectangular()
    ins, out = [lrp.Image(rect, 8, 8, 4, None)] * 2, lrp.Image(pano, 16, 8, 4, None)
    host_np, host_t = np.zeros((8, 8, 4), np.uint8), torch.zeros((8, 8, 4), dtype=torch.uint8)
    out_np, out_t = np.zeros((8, 16, 4), np.uint8), torch.zeros((8, 16, 4), dtype=torch.uint8)
    # device tensors only: host arrays and host tensors are refused in Python, whichever source carries them
    for datas, o in (([host_np, host_np], out_np), ([host_t, host_t], out_t), ([host_t, host_np], out_t)):
        with pytest.raises(ValueError, match="device tensors only"):
            lrp.compose_packed(ins, U8, datas, out, U8, o, 255, 2)
    with pytest.raises(ValueError, match="2 source images but 1 packed tensors"):
        lrp.compose_packed(ins, U8, [host_t], out, U8, out_t, 255, 2)


class _FakeCuda:
    """What compose_packed() asks of a tensor, without a device: for the checks that come after `is_cuda`."""

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
    """Element size against the format, numel against the image, one packed channel count, and the count tensor — for every
    source, not the first alone; no data_ptr() is taken before."""
    pkg = lrp
    monkeypatch.setattr(pkg, "_is_torch", lambda t: isinstance(t, _FakeCuda) or type(t).__module__.startswith("torch"))
    import torch

    rect, pano = lrp.LensInfo.rectilinear(18.0, 36.0, 8, 8), lrp.LensInfo.equirectangular()
    ins, out = [lrp.Image(rect, 8, 8, 4, None)] * 2, lrp.Image(pano, 16, 8, 4, None)
    good, good_out = _FakeCuda((8, 8, 4), 1), _FakeCuda((8, 16, 4), 1)
    with pytest.raises(ValueError, match=r"in_datas\[1\]: elements of 2 bytes"):
        lrp.compose_packed(ins, U8, [good, _FakeCuda((8, 8, 4), 2)], out, U8, good_out, 0, 2)
    with pytest.raises(ValueError, match=r"in_datas\[0\]: elements of 1 bytes"):
        lrp.compose_packed(ins, F16, [good, good], out, U8, good_out, 0, 2)
    with pytest.raises(ValueError, match="out_data: elements of 1 bytes"):
        lrp.compose_packed(ins, U8, [good, good], out, F32, good_out, 0, 2)
    with pytest.raises(ValueError, match=r"in_datas\[1\]: packed tensors must hold"):
        lrp.compose_packed(ins, U8, [good, _FakeCuda((8, 7, 4), 1)], out, U8, good_out, 0, 2)
    with pytest.raises(ValueError, match="out_data: packed tensors must hold"):
        lrp.compose_packed(ins, U8, [good, good], out, U8, _FakeCuda((8, 8, 4), 1), 0, 2)
    with pytest.raises(ValueError, match="same number of packed channels"):
        lrp.compose_packed(ins, U8, [good, _FakeCuda((8, 8, 3), 1)], out, U8, good_out, 0, 2)
    for bad in (torch.zeros((8, 16), dtype=torch.float32), torch.zeros((8, 16), dtype=torch.int8), torch.zeros((8, 15), dtype=torch.uint8),
                torch.zeros((8, 16), dtype=torch.uint8), np.zeros((8, 16), dtype=np.uint8)):  # (the last two: not device tensors)
        with pytest.raises(ValueError, match="count must be"):
            lrp.compose_packed(ins, U8, [good, good], out, U8, good_out, 0, 2, count=bad)


# ------------------------------------------------------------------ every case discriminates
def _discriminates(lrp, oracle, s, what, stats):
    packed = cp.make_inputs(s)
    for interp in (0, 1, 2):
        parts = cp.cpu_parts(lrp, s, packed, interp)
        for mode in cs.MODES:
            got, k = cp.cpu_chain(lrp, oracle, s, packed, mode, interp, parts=parts)
            ow, oh = s["case"]["out_size"]
            assert got.shape == (oh, ow, s["out_pch"]) and got.dtype == cp.pc.NUMPY_TYPES[s["out_fmt"]] and k.shape == (oh, ow)
            codes = got[k >= 1][:, :min(s["C"], s["out_pch"])].reshape(-1)
            values, counts = np.unique(codes, return_counts=True)
            share = counts.max() / codes.size
            stats.append((values.size, share, codes.size, f"{what} interp {interp} {cs.MODE_NAMES[mode]}"))
            assert values.size >= 64 and share <= 0.25, (what, interp, cs.MODE_NAMES[mode], values.size, share, codes.size)
            uncovered = got[k == 0][:, :min(s["C"], s["out_pch"])]
            assert (uncovered == 0).all(), "a k == 0 pixel encodes +0.0f"


def _report(stats):
    print(f"fewest distinct codes {min(stats)[0]} ({min(stats)[3]}); largest share {max(stats, key=lambda t: t[1])[1]:.3f} "
          f"({max(stats, key=lambda t: t[1])[3]}); fewest covered samples {min(stats, key=lambda t: t[2])[2]}")


@pytest.mark.parametrize("fmt", list(cp.FORMATS))
@pytest.mark.parametrize("case", cs.CASES, ids=[c["name"] for c in cs.CASES])
def test_cases_discriminate(lrp, oracle, case, fmt):
    stats = []
    _discriminates(lrp, oracle, cp.setup(case, **cp.FORMATS[fmt]), f"{case['name']} {fmt}", stats)
    _report(stats)


@pytest.mark.parametrize("fmt", cp.CELL_FORMATS)
@pytest.mark.parametrize("out_lens", cc.OUT_LENSES)
def test_cell_cases_discriminate(lrp, oracle, out_lens, fmt):
    """Every case of the cell sweep: each is the only test of its kernel with that sampler and source format."""
    todo = [c for c in cc.cells() if c[0] == out_lens]
    assert len(todo) == 6
    stats = []
    for cell in todo:
        case = cs.cell_case(*cell)
        _discriminates(lrp, oracle, cp.setup(case, **cp.FORMATS[fmt]), f"{case['name']} {fmt}", stats)
    _report(stats)
