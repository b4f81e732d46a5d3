"""-m gpu: lrp_reproject_packed_device (include/lrp.h "packed pixels") — 8-bit and half images reprojected by one launch —
against the chain it is defined by, byte for byte: lrp_decode_pixels_device -> lrp_reproject_device -> lrp_encode_pixels_device
(tests/packed_cases.py expect_chain: three calls the library already has).  A handful of cases is also compared with the chain
on the CPU (numpy decode, the oracle, numpy threshold encode), so that the evidence is not GPU against GPU only."""
import ctypes

import numpy as np
import pytest

import cases
import coverage_cases as cc
import packed_cases as pc

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True  # (tests/conftest.py: the module runs with the product's default, the geometry cache on)

F32, F16, U8 = pc.F32, pc.F16, pc.U8


@pytest.fixture(autouse=True)
def _setup(lrp):
    prev_ext = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    prev_cache = lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    yield
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    lrp.debug_set("geo_cache", prev_cache)
    lrp.lens_extensions(prev_ext)


def _moved(lrp, before):
    now = lrp.geometry_cache_stats()
    return now["fills"] - before["fills"], now["hits"] - before["hits"]


def _check(lrp, torch, case, seed=1, stream=None):
    """Three packed launches, each byte for byte against the chain (family 0, NaNs included): one that COMPUTES the coordinates and
    fills the geometry-cache entry (mode 1), one that reads the entry the first wrote (mode 2, a GeoRead kernel without lens math)
    and one with the cache switched off (mode 0).  The chain's own lrp_reproject_device leaves an entry under the very key of the
    packed call, so the cache is released before the first packed launch — without that it would only ever read — and the
    movement of fills / hits says that each launch was the kind it is meant to be.  num_samples > 1 always computes.
    Also against the chain of the product's default kernel family, with any NaN matching any NaN: the families of
    lrp_reproject_device differ among themselves in the sign of a NaN."""
    d_in = pc.to_device(torch, pc.make_input(case, seed))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    want = pc.expect_chain(lrp, torch, case, d_in, stream=stream)
    want_default = pc.expect_chain(lrp, torch, case, d_in, stream=stream, family=None)
    torch.cuda.synchronize()
    lrp.release_cached_tables()
    cached = 1 if case["ns"] == 1 else 0
    before = lrp.geometry_cache_stats()
    got = pc.run_packed(lrp, torch, case, d_in, stream=stream)
    assert _moved(lrp, before) == (cached, 0), f"{case['name']}: the first launch did not compute and fill"
    read = pc.run_packed(lrp, torch, case, d_in, stream=stream)
    assert _moved(lrp, before) == (cached, cached), f"{case['name']}: the second launch did not read the entry"
    lrp.debug_set("geo_cache", 0)
    try:
        off = pc.run_packed(lrp, torch, case, d_in, stream=stream)
    finally:
        lrp.debug_set("geo_cache", 1)
    assert _moved(lrp, before) == (cached, cached), f"{case['name']}: geo_cache 0 looked at the cache"
    torch.cuda.synchronize()
    w = pc.tensor_bytes(want)
    for kind, t in (("computing and filling", got), ("reading", read), ("cache off", off)):
        g = pc.tensor_bytes(t)
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{case['name']} ({kind}): {bad.size} of {g.size} bytes differ from the chain; first at byte {bad[0]}: {g[bad[0]]} vs {w[bad[0]]}")
    fmt = case["out_fmt"]
    assert pc.same_values(pc.tensor_samples(got, fmt), pc.tensor_samples(want_default, fmt), fmt), f"{case['name']}: differs from the default family's chain"
    return got


@pytest.mark.parametrize("case", pc.CASES + pc.TINY_CASES, ids=[c["name"] for c in pc.CASES + pc.TINY_CASES])
def test_cases_equal_the_chain(lrp, torch_cuda, case):
    got = _check(lrp, torch_cuda, case)
    # the same geometry on other pixels
    _check(lrp, torch_cuda, case, seed=2)
    assert tuple(got.shape) == (case["out_size"][1], case["out_size"][0], case["out_pch"])


@pytest.mark.parametrize("out_lens", cc.OUT_LENSES)
def test_every_cell_sampler_and_source_format(lrp, torch_cuda, out_lens):
    """The 30 cells x 3 samplers x {8-bit, half} source, 33 x 9 out of 21 x 13, without a rotation, with a general one and with the
    view turned round (tests/packed_cases.py CELL_ROTATIONS; one combination is left out there, with its reason).  Each case
    launches its cell's computing kernel twice (filling the entry, and with the cache off) and the GeoRead kernel once: _check."""
    todo = [c for c in pc.cell_cases() if c["out"] == out_lens]
    assert len(todo) == 6 * 3 * 2 * 3 - (6 if out_lens == pc.CELL_LEFT_OUT[0] else 0)
    for case in todo:
        _check(lrp, torch_cuda, case)


CPU_CASES = ["png_rgba8_c3_fill255", "rgba8_c4", "half_c5", "in_packed_below_c", "f16_to_u8", "u8_to_f32", "f16_to_f32", "ns2_bicubic_tonemap", "seam_7x4"]


@pytest.mark.parametrize("name", CPU_CASES)
def test_cases_equal_the_chain_on_the_cpu(lrp, oracle, torch_cuda, name):
    torch = torch_cuda
    case = next(c for c in pc.CASES if c["name"] == name)
    packed = pc.make_input(case)
    want = pc.cpu_chain(lrp, oracle, case, packed)
    got = pc.run_packed(lrp, torch, case, pc.to_device(torch, packed))
    torch.cuda.synchronize()
    assert pc.same_values(pc.tensor_samples(got, case["out_fmt"]), want, case["out_fmt"]), name


def test_python_mirror_checks_the_sample_size(lrp, torch_cuda):
    """A tensor whose elements are not the format's samples would be read or written past its end: refused before the call."""
    torch = torch_cuda
    case = pc.CASES[0]
    lin, lout = pc.lenses(lrp, case)
    (iw, ih), (ow, oh), C = case["in_size"], case["out_size"], case["C"]
    ins, out = lrp.Image(lin, iw, ih, C, None), lrp.Image(lout, ow, oh, C, None)
    u8_in = torch.zeros((ih, iw, 4), dtype=torch.uint8, device="cuda")
    for in_fmt, out_fmt, out_dtype in ((F16, U8, torch.uint8), (U8, F32, torch.uint8), (U8, F32, torch.int16), (U8, F16, torch.float32)):
        with pytest.raises(ValueError, match="-byte samples"):
            lrp.reproject_packed(ins, in_fmt, u8_in, out, out_fmt, torch.zeros((oh, ow, 4), dtype=out_dtype, device="cuda"), 0, 1, 2)


def test_num_samples_zero_leaves_the_output_untouched(lrp, torch_cuda):
    torch = torch_cuda
    case = dict(pc.CASES[0], ns=0)
    out = pc.run_packed(lrp, torch, case, pc.to_device(torch, pc.make_input(case)))
    torch.cuda.synchronize()
    assert (pc.tensor_bytes(out) == 0x5A).all()


OFFSET_CASES = ["png_rgba8_c3_fill255", "half_rgba", "rgb8_pitch3", "u8_to_f32", "f16_to_u8", "gray8", "half_c5"]


@pytest.mark.parametrize("name", OFFSET_CASES)
def test_base_pointers_at_byte_offsets_0_to_3(lrp, torch_cuda, name):
    """Source and destination at byte offsets 0-3 from an aligned address: the wide loads and stores apply only where the base is
    aligned to them, everything else goes sample by sample.  64 guard bytes either side of the output stay as they were."""
    torch = torch_cuda
    case = next(c for c in pc.CASES if c["name"] == name)
    lib = lrp._native.load()
    lin, lout = pc.lenses(lrp, case)
    (iw, ih), (ow, oh), C = case["in_size"], case["out_size"], case["C"]
    packed = pc.make_input(case)
    want = pc.tensor_bytes(pc.expect_chain(lrp, torch, case, pc.to_device(torch, packed)))
    src_bytes = torch.from_numpy(pc.as_bytes(packed).copy()).cuda()
    n_in, n_out, guard = src_bytes.numel(), want.size, 64
    rot = cases.rotation(lrp, case["deg"])
    cin, cout = lrp.Image(lin, iw, ih, C, None).to_c(), lrp.Image(lout, ow, oh, C, None).to_c()
    post = lrp._native.LrpPost(*case["post"]) if case["post"] is not None else None
    for s_off in range(4):
        d_src = torch.zeros(n_in + 8, dtype=torch.uint8, device="cuda")
        assert d_src.data_ptr() % 16 == 0
        d_src[s_off:s_off + n_in] = src_bytes
        for d_off in range(4):
            d_dst = torch.full((guard + 4 + n_out + guard,), 0xA5, dtype=torch.uint8, device="cuda")
            assert d_dst.data_ptr() % 16 == 0
            first = guard + d_off  # (guard is a multiple of 16: the offset of the base is d_off)
            cin.data, cout.data = d_src.data_ptr() + s_off, d_dst.data_ptr() + first
            st = lib.lrp_reproject_packed_device(ctypes.byref(cin), case["in_fmt"], case["in_pch"], ctypes.byref(cout), case["out_fmt"], case["out_pch"],
                                                 case["fill"], case["ns"], case["interp"], rot.ctypes.data if rot is not None else None,
                                                 ctypes.byref(post) if post is not None else None, 0, torch.cuda.current_stream().cuda_stream)
            assert st == 0, lib.lrp_last_error().decode()
            torch.cuda.synchronize()
            got = d_dst.cpu().numpy()
            assert np.array_equal(got[first:first + n_out], want), (name, s_off, d_off)
            assert (got[:first] == 0xA5).all() and (got[first + n_out:] == 0xA5).all(), (name, s_off, d_off, "guard bytes written")


def _cache_case(interp):
    return pc._case(f"cache_{interp}", "eqr_full", (64, 32), "rect18", (80, 48), pc.GENERAL, 4, U8, 4, U8, 4, fill=255, interp=interp)


@pytest.mark.parametrize("interp", [0, 1, 2])
def test_cache_fill_read_and_off_give_identical_bytes(lrp, torch_cuda, interp):
    torch = torch_cuda
    case = _cache_case(interp)
    d_in = pc.to_device(torch, pc.make_input(case))
    other = pc.to_device(torch, pc.make_input(case, seed=7))
    want = pc.tensor_bytes(pc.expect_chain(lrp, torch, dict(case), d_in))
    lrp.release_cached_tables()  # (the chain's reproject() may have made the entry)
    before = lrp.geometry_cache_stats()
    filled = pc.tensor_bytes(pc.run_packed(lrp, torch, case, d_in))
    assert _moved(lrp, before) == (1, 0)
    pc.run_packed(lrp, torch, case, other)  # other pixels in between: the geometry is what is cached
    read = pc.tensor_bytes(pc.run_packed(lrp, torch, case, d_in))
    assert _moved(lrp, before) == (1, 2)
    # num_samples > 1 always computes
    pc.run_packed(lrp, torch, dict(case, ns=2), d_in)
    assert _moved(lrp, before) == (1, 2)
    # the debug switch, then the cache itself switched off: no entry is looked at
    lrp.debug_set("geo_cache", 0)
    knob_off = pc.tensor_bytes(pc.run_packed(lrp, torch, case, d_in))
    lrp.debug_set("geo_cache", 1)
    assert _moved(lrp, before) == (1, 2)
    lrp.geometry_cache_configure(0, 1)
    cache_off = pc.tensor_bytes(pc.run_packed(lrp, torch, case, d_in))
    assert lrp.geometry_cache_stats()["entries"] == 0
    for name, got in (("fill", filled), ("read", read), ("geo_cache 0", knob_off), ("cache off", cache_off)):
        assert np.array_equal(got, want), name


@pytest.mark.parametrize("interp", [1, 2])
def test_cache_entries_are_shared_with_reproject_device(lrp, torch_cuda, interp):
    """An entry lrp_reproject_device wrote is read by the packed call, and the reverse."""
    torch = torch_cuda
    case = _cache_case(interp)
    lin, lout = pc.lenses(lrp, case)
    (iw, ih), (ow, oh) = case["in_size"], case["out_size"]
    rot = cases.rotation(lrp, case["deg"])
    d_in = pc.to_device(torch, pc.make_input(case))
    f_in = torch.rand((ih, iw, 4), dtype=torch.float32, device="cuda")

    def render_float():
        out = torch.full((oh, ow, 4), -1.0, dtype=torch.float32, device="cuda")
        lrp.reproject(lrp.Image(lin, iw, ih, 4, f_in), lrp.Image(lout, ow, oh, 4, out), 1, interp, rot)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    want_packed = pc.tensor_bytes(pc.expect_chain(lrp, torch, case, d_in))
    lrp.debug_set("geo_cache", 0)
    want_float = render_float()
    lrp.debug_set("geo_cache", 1)
    lrp.release_cached_tables()
    # lrp_reproject_device writes, the packed call reads
    before = lrp.geometry_cache_stats()
    cases.assert_same_bits(render_float(), want_float, "float fill")
    assert _moved(lrp, before) == (1, 0)
    got = pc.tensor_bytes(pc.run_packed(lrp, torch, case, d_in))
    assert _moved(lrp, before) == (1, 1) and np.array_equal(got, want_packed)
    # the packed call writes, lrp_reproject_device reads (the window kernel of a bicubic call first adds its block records to the
    # entry — a fill of its own — and reads from then on)
    lrp.release_cached_tables()
    before = lrp.geometry_cache_stats()
    got = pc.tensor_bytes(pc.run_packed(lrp, torch, case, d_in))
    assert _moved(lrp, before) == (1, 0) and np.array_equal(got, want_packed)
    cases.assert_same_bits(render_float(), want_float, "float launch on the packed call's entry")
    assert _moved(lrp, before) == ((1, 1) if interp == 1 else (2, 0))
    cases.assert_same_bits(render_float(), want_float, "float launch on the packed call's entry, again")
    assert _moved(lrp, before) == ((1, 2) if interp == 1 else (2, 1))
    assert lrp.geometry_cache_stats()["entries"] == 1


def test_side_stream(lrp, torch_cuda):
    torch = torch_cuda
    side = torch.cuda.Stream()
    for name in ("rgba8_c4", "half_rgba"):
        _check(lrp, torch, next(c for c in pc.CASES if c["name"] == name), stream=side)


def test_one_1024_frame_of_the_headline_geometry(lrp, torch_cuda):
    """BASELINE configs[1] — a 180 degree fisheye into an 18 mm view, bicubic, RGBA — at 1024^2, RGBA8 in and out: 4096 tiles,
    every XCD band; a computing launch that fills the entry, a reading one and one with the cache off (_check)."""
    case = pc._case("config1_1024", "eqd_pi", (1024, 1024), "rect18", (1024, 1024), None, 4, U8, 4, U8, 4)
    _check(lrp, torch_cuda, case)
    _check(lrp, torch_cuda, case, seed=3)
