"""CPU: supersampled compose (include/lrp.h "compose, supersampled") without a GPU — the CPU model the GPU tests compare with
(tests/native/compose_ss_model.c) is the definition: its n = 1 output is the composition helper of tests/compose_cases.py on the
coverage model's parts, its coverage plane the per-sub-sample definition, its single-source full-coverage pixels the coverage
model's supersampled render; the cases of tests/compose_ss_cases.py discriminate; the seam counts of the cube; and the argument
errors of lrp_compose_ss_device, each before any device call."""
import ctypes

import numpy as np
import pytest

import cases
import compose_cases as cs
import compose_ss_cases as ss
import compose_ss_model as ssm
import coverage_cases as cc
import coverage_model as model


@pytest.fixture(autouse=True)
def extensions_on(lrp):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    try:
        yield
    finally:
        lrp.lens_extensions(prev)


def model_compose(lrp, case, n, interp, mode, srcs, post=None):
    lout, lins = cs.lenses(lrp, case)
    ow, oh = case["out_size"]
    return ssm.compose(lins, srcs, lout, ow, oh, n, interp, ss.rotations(lrp, case), mode, post)


# ------------------------------------------------------------------ 1. the model is the definition
@pytest.mark.parametrize("case", cs.OVERLAP_CASES, ids=[c["name"] for c in cs.OVERLAP_CASES])
def test_n1_is_compose(lrp, case):
    """n = 1: the image and the count plane of compose_cases.expect() on the coverage model's per-source renders, planes and
    weights, all three modes and samplers; coverage is k > 0.  (The noise sources have no zero texel: no -0.0 arises.)"""
    lout, lins = cs.lenses(lrp, case)
    ow, oh = case["out_size"]
    srcs = ss.sources(case)
    for interp in (0, 1, 2):
        renders, planes, weights = [], [], []
        for lin, src, (name, (w, h), deg) in zip(lins, srcs, case["sources"]):
            rot = cases.rotation(lrp, deg)
            renders.append(model.reproject(lin, src, lout, ow, oh, 1, interp, rot))
            plane, sxy, _ = model.coverage(lin, w, h, lout, ow, oh, 1, rot, detail=True)
            planes.append(plane)
            weights.append(cs.feather_weight(sxy[:, :, 0, :], w, h, cs.wraps(name)))
        for mode in cs.MODES:
            want, k = cs.expect(mode, renders, planes, weights)
            got, count, coverage = model_compose(lrp, case, 1, interp, mode, srcs)
            cases.assert_same_bits(got, want, f"{case['name']} {cs.MODE_NAMES[mode]} interp {interp}")
            assert (count == k).all() and (coverage == (k > 0)).all()


@pytest.mark.parametrize("item", ss.DISCRIMINATING, ids=ss.case_id)
def test_planes_are_the_definition_per_sub_sample(lrp, item):
    case, n = item
    count, m = ss.planes(ss.sub_covered(lrp, case, n))
    for mode in cs.MODES:
        _, got_count, got_m = model_compose(lrp, case, n, 0, mode, ss.sources(case, channels=1))
        assert (got_m == m).all() and (got_count == count).all(), cs.MODE_NAMES[mode]


@pytest.mark.parametrize("n", [2, 3, 4])
def test_one_source_fully_covered_pixels_are_the_supersampled_render(lrp, n):
    """One source, FIRST and MEAN: where m == n * n the pixel is what the coverage model's n-sample reproject() renders."""
    case = cs._case("one", "eqr_full", (96, 48), [("rect18", (64, 48), cc.GENERAL)])
    lout, lins = cs.lenses(lrp, case)
    srcs = ss.sources(case)
    rot = cases.rotation(lrp, cc.GENERAL)
    for interp in (0, 1, 2):
        want = model.reproject(lins[0], srcs[0], lout, 96, 48, n, interp, rot)
        for mode in (cs.FIRST, cs.MEAN):
            got, count, m = model_compose(lrp, case, n, interp, mode, srcs)
            full = m == n * n
            assert 0.05 < full.mean() < 0.95 and ((m > 0) & ~full).any()
            cases.assert_same_bits(got[full], want[full], f"n {n} interp {interp} {cs.MODE_NAMES[mode]}")
            assert (got[m == 0].view(np.uint32) == 0).all() and (count == (m > 0)).all()


def test_post_touches_the_covered_pixels_only(lrp):
    case = cs.OVERLAP_CASES[0]
    for channels in (2, 5):
        srcs = ss.sources(case, channels=channels)
        plain, _, m = model_compose(lrp, case, 2, 1, cs.FEATHER, srcs)
        toned, _, m2 = model_compose(lrp, case, 2, 1, cs.FEATHER, srcs, post=(2.0, 3.0))
        want = np.ascontiguousarray(plain.copy())
        img = lrp.LensInfo.equirectangular()
        import oracle_binding as oracle

        cimg = oracle._image(img, want.shape[1], want.shape[0], channels, want)
        model.lib().cvm_post_process(ctypes.byref(cimg), 2.0, 3.0)
        cases.assert_same_bits(toned[m > 0], want[m > 0], f"post, C {channels}")
        assert (toned[m == 0].view(np.uint32) == 0).all() and (m == m2).all() and (m == 0).any()


# ------------------------------------------------------------------ 2. the cases discriminate
@pytest.mark.parametrize("item", ss.DISCRIMINATING, ids=ss.case_id)
def test_cases_discriminate(lrp, item):
    case, n = item
    partial, differs = ss.fractions(ss.sub_covered(lrp, case, n))
    print(f"{ss.case_id(item)}: 0 < m < n * n in {partial:.4f} of the pixels, the covering set differs in {differs:.4f}")
    assert partial >= ss.PARTIAL_MIN and differs >= ss.SET_DIFFERS_MIN


@pytest.mark.parametrize("item", ss.NOT_DISCRIMINATING, ids=ss.case_id)
def test_the_excluded_cases_are_the_ones_that_do_not(lrp, item):
    """eqs2_pano at n = 2 and 3: the boundaries fall between pixel columns; nothing here would be lost by leaving it out."""
    case, n = item
    assert ss.fractions(ss.sub_covered(lrp, case, n)) == (0.0, 0.0)


CELLS = cc.cells()


@pytest.mark.parametrize("cell", CELLS, ids=[f"{o}<-{s}" for o, s, _ in CELLS])
def test_cells_discriminate(lrp, cell):
    for n in ss.CELL_N:
        _, differs = ss.fractions(ss.sub_covered(lrp, cs.cell_case(*cell), n))
        print(f"{cell} n {n}: the covering set differs in {differs:.4f} of the pixels")
        assert differs >= ss.CELL_SET_DIFFERS_MIN


def test_supersampling_differs_from_a_larger_render_shrunk(lrp):
    """The modes differ where sources overlap, and n = 2 is not n = 1: the sub-sample positions decide."""
    case = cs.OVERLAP_CASES[0]
    srcs = ss.sources(case)
    one, _, _ = model_compose(lrp, case, 1, 1, cs.MEAN, srcs)
    two, count, m = model_compose(lrp, case, 2, 1, cs.MEAN, srcs)
    first, _, _ = model_compose(lrp, case, 2, 1, cs.FIRST, srcs)
    feather, _, _ = model_compose(lrp, case, 2, 1, cs.FEATHER, srcs)
    assert (~cases.same_bits(one, two)).any(axis=2)[m > 0].mean() > 0.9
    assert (~cases.same_bits(two, first)).any(axis=2)[count >= 2].mean() > 0.5 and (~cases.same_bits(two, feather)).any(axis=2)[count >= 2].mean() > 0.5
    cases.assert_same_bits(two[count == 1], first[count == 1], "MEAN of one source")


def test_cube_seam_counts(lrp):
    """Six 90 x 90 degree faces into 128 x 64: the 14 pixels no face covers at n = 1 (binary32 cracks at the seams, DESIGN.md
    section 12) are gone at n = 2 — a pixel is uncovered only if all its sub-samples fall into a crack.  The model's counts are
    the figures of DESIGN.md section 16; the GPU test asserts the same numbers."""
    cov1 = ss.sub_covered(lrp, cs.CUBE, 1)
    assert int((ss.planes(cov1)[1] == 0).sum()) == cs.CUBE_SEAMS["k0"]
    count, m = ss.planes(ss.sub_covered(lrp, cs.CUBE, 2))
    want = ss.CUBE_SEAMS_N2
    assert int((m == 0).sum()) == want["m0"] and int(((m > 0) & (m < 4)).sum()) == want["partial"] and int((count >= 2).sum()) == want["count2"]
    _, got_count, got_m = model_compose(lrp, cs.CUBE, 2, 0, cs.FIRST, ss.sources(cs.CUBE, channels=1))
    assert (got_m == m).all() and (got_count == count).all()


# ------------------------------------------------------------------ 3. argument errors (no device is touched before them)
def _status(lrp, lenses, lout, n, mode=0, interp=2, channels=None, planes=False):
    lib = lrp._native.load()
    k = len(lenses)
    channels = channels or [4] * k
    arr = (lrp._native.LrpImage * max(k, 1))()
    for i, lin in enumerate(lenses):
        arr[i] = lrp.Image(lin, 8, 8, channels[i], None).to_c()
        arr[i].data = 0x1000  # never dereferenced: every call here fails, in validation or at device -1
    cout = lrp.Image(lout, 8, 8, 4, None).to_c()
    cout.data = 0x2000
    st = lib.lrp_compose_ss_device(arr, k, None, ctypes.byref(cout), n, interp, mode, None, 0x3000 if planes else None,
                                   0x4000 if planes else None, -1, None)
    return st, lib.lrp_last_error().decode()


def test_argument_errors(lrp):
    S = lrp.Status
    L = lrp.LensInfo
    rect, pano = L.rectilinear(18.0, 36.0, 8, 8), L.equirectangular()
    for n in (0, -1, 16):
        st, text = _status(lrp, [rect, rect], pano, n)
        assert st == S.BAD_ARG and "num_samples" in text
    # compose's own errors come first, in compose's order
    assert _status(lrp, [], pano, 0)[0] == S.BAD_ARG and "n_in" in _status(lrp, [], pano, 0)[1]
    assert "n_in" in _status(lrp, [rect] * 9, pano, 16)[1]
    assert "mode" in _status(lrp, [rect], pano, 0, mode=3)[1]
    assert _status(lrp, [rect] * 2, pano, 0, interp=3)[0] == S.INTERPOLATION
    assert _status(lrp, [rect, rect], pano, 16, channels=[4, 3])[0] == S.CHANNELS
    st, text = _status(lrp, [rect, L.equidistant(3.0)], pano, 0)
    assert st == S.BAD_ARG and "rectilinear" in text and "equidistant" in text
    lrp.lens_extensions(0)
    assert _status(lrp, [L.equisolid(10.0, 36.0, 3.0, 8, 8)], pano, 0)[0] == S.INPUT_LENS
    lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    # good calls get as far as the device: every n of 1 .. 15, every mode, with and without planes
    for n in range(1, 16):
        assert _status(lrp, [rect, rect], pano, n, mode=n % 3, planes=bool(n % 2))[0] == S.NO_DEVICE
    assert "lrp_compose_ss_device" in lrp._native.SYMBOLS
    assert lrp._native.load().lrp_abi_version() == 3


def test_plane_tensors_are_checked_in_python(lrp):
    import torch

    rect, pano = lrp.LensInfo.rectilinear(18.0, 36.0, 8, 8), lrp.LensInfo.equirectangular()
    ins, out = [lrp.Image(rect, 8, 8, 4, None)], lrp.Image(pano, 16, 8, 4, None)
    host_in, host_out = np.zeros((8, 8, 4), dtype=np.float32), np.zeros((8, 16, 4), dtype=np.float32)
    for bad_ins, bad_out in (([lrp.Image(rect, 8, 8, 4, host_in)], lrp.Image(pano, 16, 8, 4, host_out)),
                             ([lrp.Image(rect, 8, 8, 4, torch.from_numpy(host_in))], lrp.Image(pano, 16, 8, 4, torch.from_numpy(host_out))),
                             (ins, out)):
        with pytest.raises(ValueError, match="device tensors only"):
            lrp.compose_ss(bad_ins, bad_out, 2, 2)
    for bad in (torch.zeros((8, 16), dtype=torch.float32), torch.zeros((8, 16), dtype=torch.int8), torch.zeros((8, 15), dtype=torch.uint8),
                torch.zeros((8, 16), dtype=torch.uint8), np.zeros((8, 16), dtype=np.uint8)):  # (the last two: not device tensors)
        with pytest.raises(ValueError, match="count must be"):
            lrp.compose_ss(ins, out, 2, 2, count=bad)
        with pytest.raises(ValueError, match="coverage must be"):
            lrp.compose_ss(ins, out, 2, 2, coverage=bad)
