"""CPU: the cases of the compose tests (tests/compose_cases.py) discriminate — by the coverage model (tests/coverage_model.py),
which tests/test_coverage.py pins to the definition —, the seam counts of the cube case, the composition helper against a
per-pixel restatement, and the argument errors of lrp_compose_device, each before any device call."""
import ctypes

import numpy as np
import pytest

import cases
import compose_cases as cs
import coverage_model as model


@pytest.fixture(autouse=True)
def extensions_on(lrp):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    try:
        yield
    finally:
        lrp.lens_extensions(prev)


def model_parts(lrp, case, channels=4, interp=0, seed=100):
    """Per source: the model's render, coverage plane and feather weight."""
    lout, lins = cs.lenses(lrp, case)
    ow, oh = case["out_size"]
    renders, planes, weights = [], [], []
    for i, (lin, (name, (w, h), deg)) in enumerate(zip(lins, case["sources"])):
        rot = cases.rotation(lrp, deg)
        src = cases.hash_noise(h, w, channels, seed + i, planted=False)
        renders.append(model.reproject(lin, src, lout, ow, oh, 1, interp, rot))
        plane, sxy, _ = model.coverage(lin, w, h, lout, ow, oh, 1, rot, detail=True)
        planes.append(plane)
        weights.append(cs.feather_weight(sxy[:, :, 0, :], w, h, cs.wraps(name)))
    return renders, planes, weights


@pytest.mark.parametrize("case", cs.OVERLAP_CASES, ids=[c["name"] for c in cs.OVERLAP_CASES])
def test_overlap_cases_discriminate(lrp, case):
    renders, planes, weights = model_parts(lrp, case)
    first, k = cs.expect(cs.FIRST, renders, planes)
    k0, k1, k2 = (k == 0).mean(), (k == 1).mean(), (k >= 2).mean()
    print(f"{case['name']}: k = 0 {k0:.3f}, k = 1 {k1:.3f}, k >= 2 {k2:.3f}")
    assert k0 >= 0.05 and k1 >= 0.05 and k2 >= 0.05, (k0, k1, k2)
    reversed_first, _ = cs.expect(cs.FIRST, renders[::-1], planes[::-1])
    differs = (~cases.same_bits(first, reversed_first)).any(axis=2).mean()
    print(f"{case['name']}: FIRST in reversed order differs in {differs:.3f} of the pixels")
    assert differs >= 0.01
    # the three modes are three different images where sources overlap, and the same image where one source covers
    mean, _ = cs.expect(cs.MEAN, renders, planes)
    feather, _ = cs.expect(cs.FEATHER, renders, planes, weights)
    assert (~cases.same_bits(first, mean)).any(axis=2)[k >= 2].mean() > 0.5 and (~cases.same_bits(mean, feather)).any(axis=2)[k >= 2].mean() > 0.5
    cases.assert_same_bits(mean[k == 1], first[k == 1], "MEAN of one source")
    assert (first[k == 0] == 0).all() and (mean[k == 0] == 0).all() and (feather[k == 0] == 0).all() and not np.signbit(feather[k == 0]).any()


def test_cube_seam_counts(lrp):
    """Six 90 x 90 degree faces into a 128 x 64 panorama: rounding at the seams leaves pixels that no face covers and pixels that
    two cover.  The model's counts are the figures of DESIGN.md section 12 (the GPU test asserts the same two numbers)."""
    _, planes, _ = model_parts(lrp, cs.CUBE, channels=1)
    k = np.sum([p > 0 for p in planes], axis=0)
    assert int((k == 0).sum()) == cs.CUBE_SEAMS["k0"] and int((k >= 2).sum()) == cs.CUBE_SEAMS["k2"]
    assert k.max() == 2


def test_expect_is_the_definition_pixel_by_pixel(lrp):
    """The vectorised helper against the loops of include/lrp.h "compose", written out per pixel."""
    case = cs.OVERLAP_CASES[0]
    renders, planes, weights = model_parts(lrp, case, channels=3)
    oh, ow, C = renders[0].shape
    for mode in cs.MODES:
        got, k = cs.expect(mode, renders, planes, weights)
        want = np.zeros((oh, ow, C), dtype=np.float32)
        for y in range(oh):
            for x in range(ow):
                cover = [i for i in range(len(planes)) if planes[i][y, x] > 0]
                assert k[y, x] == len(cover)
                if not cover:
                    continue
                if mode == cs.FIRST:
                    want[y, x] = renders[cover[0]][y, x]
                    continue
                acc, wsum = np.zeros(C, dtype=np.float32), np.float32(0.0)
                for i in cover:
                    w = weights[i][y, x] if mode == cs.FEATHER else np.float32(1.0)
                    acc = acc + (w * renders[i][y, x] if mode == cs.FEATHER else renders[i][y, x])
                    wsum = wsum + w
                want[y, x] = acc / (np.float32(len(cover)) if mode == cs.MEAN else wsum)
        cases.assert_same_bits(got, want, cs.MODE_NAMES[mode])


def test_single_source_first_is_the_masked_render(lrp):
    case = cs._case("one", "eqr_full", (96, 48), [("rect18", (64, 48), (30.0, -15.0, 5.0))])
    renders, planes, _ = model_parts(lrp, case)
    got, k = cs.expect(cs.FIRST, renders, planes)
    cases.assert_same_bits(got, model.masked(renders[0], planes[0]), "n_in = 1")
    assert (k == planes[0]).all()


# ------------------------------------------------------------------ argument errors (no device is touched before them)
def _status(lrp, lenses, lout, mode=0, interp=2, channels=None, out_channels=4, rotations=False):
    lib = lrp._native.load()
    n = len(lenses)
    channels = channels or [4] * n
    arr = (lrp._native.LrpImage * max(n, 1))()
    for i, lin in enumerate(lenses):
        arr[i] = lrp.Image(lin, 8, 8, channels[i], None).to_c()
        arr[i].data = 0x1000  # never dereferenced: every call here fails, in validation or at device -1
    cout = lrp.Image(lout, 8, 8, out_channels, None).to_c()
    cout.data = 0x2000
    rot = np.tile(np.eye(3, dtype=np.float32).reshape(9), max(n, 1)) if rotations else None
    st = lib.lrp_compose_device(arr, n, rot.ctypes.data if rotations else None, ctypes.byref(cout), interp, mode, None, None, -1, None)
    return st, lib.lrp_last_error().decode()


def test_argument_errors(lrp):
    S = lrp.Status
    L = lrp.LensInfo
    rect, pano = L.rectilinear(18.0, 36.0, 8, 8), L.equirectangular()
    assert _status(lrp, [], pano)[0] == S.BAD_ARG
    assert _status(lrp, [rect] * 9, pano)[0] == S.BAD_ARG
    assert _status(lrp, [rect] * 2, pano, mode=3)[0] == S.BAD_ARG and _status(lrp, [rect], pano, mode=-1)[0] == S.BAD_ARG
    assert _status(lrp, [rect] * 2, pano, interp=3)[0] == S.INTERPOLATION
    assert _status(lrp, [rect, rect], pano, channels=[4, 3])[0] == S.CHANNELS
    assert _status(lrp, [rect, rect], pano, channels=[3, 3], out_channels=4)[0] == S.CHANNELS
    # mixed source modes: the text names both; clamped and wrapping equirectangular sources are two modes
    st, text = _status(lrp, [rect, L.equidistant(3.0)], pano)
    assert st == S.BAD_ARG and "rectilinear" in text and "equidistant" in text
    st, text = _status(lrp, [pano, L.equirectangular(-1.0, 1.0, -0.5, 0.5)], rect)
    assert st == S.BAD_ARG and "wrapping equirectangular" in text and "clamped equirectangular" in text
    # n_in and mode come before the per-source checks, those before the mode mix
    assert _status(lrp, [L.equidistant(3.0)] * 9, pano, interp=7)[0] == S.BAD_ARG
    assert _status(lrp, [rect, L.equidistant(3.0)], pano, channels=[4, 2])[0] == S.CHANNELS
    # good calls get as far as the device: every mode, 1 and 8 sources, with and without rotations
    for mode in cs.MODES:
        assert _status(lrp, [rect], pano, mode=mode)[0] == S.NO_DEVICE
    assert _status(lrp, [rect] * 8, pano, rotations=True)[0] == S.NO_DEVICE
    assert _status(lrp, [L.equirectangular(-1.0, 1.0, -0.5, 0.5), L.equirectangular(-2.0, 0.5, -0.2, 0.5)], rect)[0] == S.NO_DEVICE
    assert lrp.COMPOSE_MAX_SOURCES == 8 and [int(m) for m in lrp.ComposeMode] == [0, 1, 2]
    assert "lrp_compose_device" in lrp._native.SYMBOLS
    assert lrp._native.load().lrp_abi_version() == 3


def test_extension_lenses_need_their_bit(lrp):
    S = lrp.Status
    L = lrp.LensInfo
    rect, pano = L.rectilinear(18.0, 36.0, 8, 8), L.equirectangular()
    eqs, stg = L.equisolid(10.0, 36.0, 3.0, 8, 8), L.stereographic(10.0, 36.0, 8, 8)
    assert _status(lrp, [eqs, eqs], pano)[0] == S.NO_DEVICE and _status(lrp, [stg], stg)[0] == S.NO_DEVICE
    lrp.lens_extensions(lrp.LENS_EXT_STEREOGRAPHIC)
    assert _status(lrp, [eqs, eqs], pano)[0] == S.INPUT_LENS and _status(lrp, [rect], eqs)[0] == S.OUTPUT_LENS
    assert _status(lrp, [rect, eqs], pano)[0] == S.INPUT_LENS  # (the second source's lens check comes before the mode mix)
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID)
    assert _status(lrp, [stg, stg], pano)[0] == S.INPUT_LENS and _status(lrp, [rect], stg)[0] == S.OUTPUT_LENS
    lrp.lens_extensions(0)
    assert _status(lrp, [eqs], pano)[0] == S.INPUT_LENS and _status(lrp, [stg], pano)[0] == S.INPUT_LENS


def test_count_tensor_is_checked_in_python(lrp):
    import torch

    rect, pano = lrp.LensInfo.rectilinear(18.0, 36.0, 8, 8), lrp.LensInfo.equirectangular()
    ins, out = [lrp.Image(rect, 8, 8, 4, None)], lrp.Image(pano, 16, 8, 4, None)
    # device tensors only: host arrays, host tensors and missing data are refused in Python, before any pointer reaches the library
    host_in, host_out = np.zeros((8, 8, 4), dtype=np.float32), np.zeros((8, 16, 4), dtype=np.float32)
    for bad_ins, bad_out in (([lrp.Image(rect, 8, 8, 4, host_in)], lrp.Image(pano, 16, 8, 4, host_out)),
                             ([lrp.Image(rect, 8, 8, 4, torch.from_numpy(host_in))], lrp.Image(pano, 16, 8, 4, torch.from_numpy(host_out))),
                             (ins, out)):
        with pytest.raises(ValueError, match="device tensors only"):
            lrp.compose(bad_ins, bad_out, 2)
    for bad in (torch.zeros((8, 16), dtype=torch.float32), torch.zeros((8, 16), dtype=torch.int8), torch.zeros((8, 15), dtype=torch.uint8),
                torch.zeros((8, 16), dtype=torch.uint8), np.zeros((8, 16), dtype=np.uint8)):  # (the last two: not device tensors)
        with pytest.raises(ValueError, match="count must be"):
            lrp.compose(ins, out, 2, count=bad)
