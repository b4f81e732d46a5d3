"""CPU: lrp_reproject_packed_device (include/lrp.h "packed pixels") without a device — the symbol and its Python mirror exist,
the argument errors come in the documented order with the documented statuses (all of them before a device is touched; valid
arguments get as far as LRP_ERR_NO_DEVICE), and every case of tests/packed_cases.py — the named cases and the whole cell sweep —
discriminates: the chain on the CPU — numpy decode with pixel_tables(), the oracle, numpy threshold encode — has at least 64
distinct codes per case and no code that makes up more than half of the samples.  (Not held to it: the five TINY_CASES, whose
1 x 1 or 2 x 2 source or 1 x 1 output has too few samples by construction.)"""
import ctypes
import inspect

import numpy as np
import pytest

import packed_cases as pc

F32, F16, U8 = pc.F32, pc.F16, pc.U8


def _status(lrp, lin=None, lout=None, in_fmt=U8, in_pch=4, out_fmt=U8, out_pch=4, interp=2, channels=4, out_channels=None, in_size=(8, 8),
            out_size=(8, 8), null=None, ns=1):
    L = lrp.LensInfo
    lib = lrp._native.load()
    lin = lin or L.equidistant(3.0)
    lout = lout or L.rectilinear(18.0, 36.0, *out_size)
    cin = lrp.Image(lin, in_size[0], in_size[1], channels, None).to_c()
    cout = lrp.Image(lout, out_size[0], out_size[1], channels if out_channels is None else out_channels, None).to_c()
    cin.data = None if null == "in_data" else 0x1000  # never dereferenced: every call here fails, in validation or at device -1
    cout.data = None if null == "out_data" else 0x2000
    st = lib.lrp_reproject_packed_device(None if null == "in" else ctypes.byref(cin), in_fmt, in_pch, None if null == "out" else ctypes.byref(cout),
                                         out_fmt, out_pch, 255, ns, interp, None, None, -1, None)
    return st, lib.lrp_last_error().decode()


def test_symbol_and_python_mirror_exist(lrp):
    lib = lrp._native.load()
    assert hasattr(lib, "lrp_reproject_packed_device") and "lrp_reproject_packed_device" in lrp._native.SYMBOLS
    assert lib.lrp_abi_version() == 3
    names = list(inspect.signature(lrp.reproject_packed).parameters)
    assert names == ["in_image", "in_format", "in_data", "out_image", "out_format", "out_data", "out_fill", "num_samples", "interpolation",
                     "rotation_matrix", "post", "device", "stream"]


def test_argument_errors_in_the_documented_order(lrp):
    S, L = lrp.Status, lrp.LensInfo
    eqs = L.equisolid(10.0, 36.0, 3.0, 8, 8)
    prev = lrp.lens_extensions(0)
    try:
        # 1. NULL images
        assert _status(lrp, null="in")[0] == S.NULL and _status(lrp, null="out")[0] == S.NULL
        # 2. the checks of lrp_reproject_device, in its order: output lens, input lens (extension bits), interpolation, channels,
        #    sizes, data pointers — each in front of everything behind it
        assert _status(lrp, lout=eqs, lin=eqs, interp=7, in_fmt=F32)[0] == S.OUTPUT_LENS
        assert _status(lrp, lin=eqs, interp=7, in_fmt=F32)[0] == S.INPUT_LENS
        lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID)
        assert _status(lrp, lin=eqs, lout=eqs)[0] == S.NO_DEVICE
        lrp.lens_extensions(0)
        assert _status(lrp, interp=3, channels=0, in_fmt=F32)[0] == S.INTERPOLATION
        assert _status(lrp, channels=0, in_size=(0, 8), in_fmt=9)[0] == S.CHANNELS
        assert _status(lrp, channels=4, out_channels=3, in_fmt=9)[0] == S.CHANNELS
        assert _status(lrp, in_size=(0, 8), in_fmt=9)[0] == S.BAD_DIMS and _status(lrp, out_size=(8, -1), null="in_data")[0] == S.BAD_DIMS
        assert _status(lrp, in_size=(1 << 15, 1 << 15), channels=4, in_fmt=9)[0] == S.BAD_DIMS  # 2^32 floats
        assert _status(lrp, null="in_data", in_fmt=9)[0] == S.NULL and _status(lrp, null="out_data", in_pch=0)[0] == S.NULL
        # 3. formats and packed channel counts; a float32 source names the two calls to make instead
        st, text = _status(lrp, in_fmt=F32, channels=9)
        assert st == S.BAD_ARG and "lrp_reproject_device" in text and "lrp_encode_pixels_device" in text
        assert _status(lrp, in_fmt=3, channels=9)[0] == S.BAD_ARG and _status(lrp, in_fmt=-1)[0] == S.BAD_ARG
        assert _status(lrp, out_fmt=3, channels=9)[0] == S.BAD_ARG and _status(lrp, out_fmt=-1)[0] == S.BAD_ARG
        assert _status(lrp, in_pch=0, channels=9)[0] == S.BAD_ARG and _status(lrp, out_pch=0)[0] == S.BAD_ARG and _status(lrp, in_pch=-4)[0] == S.BAD_ARG
        # 4. more than 8 channels: in front of the size check of the packed images
        assert _status(lrp, channels=9, in_size=(1 << 13, 1 << 13), in_pch=64)[0] == S.CHANNELS  # (2^32 packed bytes)
        assert _status(lrp, channels=8, in_fmt=F16, in_pch=8, out_pch=8)[0] == S.NO_DEVICE
        # 5. the packed images fit 32-bit byte offsets: 2^31 bytes is the last size that does
        assert _status(lrp, channels=1, in_size=(1 << 14, 1 << 14), in_pch=8)[0] == S.NO_DEVICE  # 2^31 bytes of 8-bit samples
        assert _status(lrp, channels=1, in_size=(1 << 14, 1 << 14), in_pch=9)[0] == S.BAD_DIMS
        assert _status(lrp, channels=1, in_size=(1 << 14, 1 << 14), in_fmt=F16, in_pch=4)[0] == S.NO_DEVICE
        assert _status(lrp, channels=1, in_size=(1 << 14, 1 << 14), in_fmt=F16, in_pch=5)[0] == S.BAD_DIMS
        assert _status(lrp, channels=1, out_size=(1 << 14, 1 << 14), out_fmt=F32, out_pch=2)[0] == S.NO_DEVICE
        st, text = _status(lrp, channels=1, out_size=(1 << 14, 1 << 14), out_fmt=F32, out_pch=3)
        assert st == S.BAD_DIMS and "2^31 bytes" in text
        assert _status(lrp, channels=1, in_size=(1 << 14, 1 << 14), in_pch=(1 << 31) - 1)[0] == S.BAD_DIMS  # (no overflow in the product)
        # valid arguments reach the device: both source formats, every output format, every sampler, num_samples <= 0 too
        for in_fmt in (F16, U8):
            for out_fmt in (F32, F16, U8):
                for interp in (0, 1, 2):
                    assert _status(lrp, in_fmt=in_fmt, out_fmt=out_fmt, interp=interp)[0] == S.NO_DEVICE
        assert _status(lrp, ns=0)[0] == S.NO_DEVICE and _status(lrp, channels=1, in_pch=7, out_pch=64)[0] == S.NO_DEVICE
    finally:
        lrp.lens_extensions(prev)


def test_python_mirror_takes_device_tensors_only(lrp):
    import torch

    rect, pano = lrp.LensInfo.rectilinear(18.0, 36.0, 8, 8), lrp.LensInfo.equirectangular()
    ins, out = lrp.Image(pano, 8, 8, 4, None), lrp.Image(rect, 8, 8, 4, None)
    for a, b in ((np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 4), np.uint8)), (torch.zeros((8, 8, 4), dtype=torch.uint8),) * 2):
        with pytest.raises(ValueError, match="device tensors only"):
            lrp.reproject_packed(ins, U8, a, out, U8, b, 255, 1, 2)


def _discriminates(lrp, oracle, case):
    packed = pc.make_input(case)
    got = pc.cpu_chain(lrp, oracle, case, packed)
    ow, oh = case["out_size"]
    assert got.shape == (oh, ow, case["out_pch"]) and got.dtype == pc.NUMPY_TYPES[case["out_fmt"]]
    codes = got[..., :min(case["C"], case["out_pch"])].reshape(-1)  # (the fill samples are one code by definition)
    codes = codes.view(np.uint32) if case["out_fmt"] == F32 else codes
    values, counts = np.unique(codes, return_counts=True)
    print(f"{case['name']}: {values.size} distinct codes in {codes.size} samples, the most frequent one {counts.max() / codes.size:.3f} of them")
    assert values.size >= 64 and counts.max() <= codes.size / 2, case["name"]


@pytest.mark.parametrize("case", pc.CASES, ids=[c["name"] for c in pc.CASES])
def test_cases_discriminate(lrp, oracle, case):
    _discriminates(lrp, oracle, case)


@pytest.mark.parametrize("out_lens", pc.cc.OUT_LENSES)
def test_cell_cases_discriminate(lrp, oracle, out_lens):
    """Every case of the cell sweep: each is the only test of its computing kernel with that sampler and source format."""
    todo = [c for c in pc.cell_cases() if c["out"] == out_lens]
    assert len(todo) == 6 * 3 * 2 * 3 - (6 if out_lens == pc.CELL_LEFT_OUT[0] else 0)
    for case in todo:
        _discriminates(lrp, oracle, case)


def test_half_cases_carry_the_planted_texels():
    n = 0
    for case in pc.CASES:
        if case["in_fmt"] != F16:
            continue
        n += 1
        packed = pc.make_input(case)
        present = set(packed.reshape(-1).tolist())
        assert set(pc.PLANTED_HALVES.tolist()) <= present, case["name"]
    assert n >= 8
    # what the list is: +0, -0, the smallest and a negative denormal, +inf, -inf, a NaN, 65504
    h = pc.PLANTED_HALVES.view(np.float16).astype(np.float32)
    assert h[0] == 0 and not np.signbit(h[0]) and h[1] == 0 and np.signbit(h[1]) and 0 < h[2] < 6.2e-5 and -6.2e-5 < h[3] < 0
    assert h[4] == np.inf and h[5] == -np.inf and np.isnan(h[6]) and h[7] == 65504.0


def test_numpy_codecs_are_the_tables(lrp):
    """decode_numpy / encode_numpy against the two tables: every byte decodes to its entry and encodes back to itself, the
    clamp sends NaN to 255 and -0 to 0."""
    dec, thr = lrp.pixel_tables()
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    f = pc.decode_numpy(lrp, ramp, U8, 3)
    assert np.array_equal(f[..., 0].reshape(-1), dec) and not f[..., 1:].any()
    assert np.array_equal(pc.encode_numpy(lrp, f, U8, 1, 0), ramp)
    odd = np.array([np.nan, -0.0, -1.0, 2.0, np.inf, -np.inf, thr[7], np.nextafter(thr[7], np.float32(0))], dtype=np.float32).reshape(1, 8, 1)
    assert pc.encode_numpy(lrp, odd, U8, 2, 9).reshape(8, 2).tolist() == [[255, 9], [0, 9], [0, 9], [255, 9], [255, 9], [0, 9], [7, 9], [6, 9]]
