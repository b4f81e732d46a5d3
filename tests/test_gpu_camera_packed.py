"""GPU: lrp_compose_cameras_packed_device and lrp_camera_overlap_packed_device (include/lrp.h "calibrated cameras, packed
pixels"; csrc/lrp_camera_packed_kernel.h, csrc/lrp_camstat_packed_kernel.h) against the chains they are defined by, run on the
GPU by the calls the library already has (tests/camera_packed_cases.py expect_chain / expect_overlap): decode per camera ->
compose_cameras(gains=) -> encode, and decode -> camera_overlap.  With an 8-bit source the comparison is strict, byte for byte,
on the output, the count plane and the coverage plane; with a half source a NaN matches a NaN.  The overlap table is compared as
integers, all 128 words.  Outputs and planes are prefilled on both sides.  tests/test_camera_packed.py shows on the CPU that the
cases discriminate."""
import math

import numpy as np
import pytest

import camera_cases as cam
import camera_gain_cases as gc
import camera_packed_cases as kp
import packed_cases as pc

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True  # (the tests set the cache themselves)
F32, F16, U8 = kp.F32, kp.F16, kp.U8
FIRST, MEAN, FEATHER = kp.FIRST, kp.MEAN, kp.FEATHER


@pytest.fixture(autouse=True)
def extensions_on(lrp, torch_cuda):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    prev_cache, prev_kernel = lrp.debug_set("geo_cache", 0), lrp.debug_kernel(-1)
    try:
        yield
    finally:
        lrp.debug_kernel(prev_kernel)
        lrp.debug_set("geo_cache", prev_cache)
        lrp.lens_extensions(prev)


def upload(torch, s, sc, packed=None):
    return [pc.to_device(torch, a) for a in (packed if packed is not None else kp.make_inputs(s, sc))]


def check(lrp, torch, s, sc, gains, n, interp, mode, what, d_ins=None, count=True, stream=None):
    """The fused call against the chain on the same device frames: the output and both planes."""
    d_ins = d_ins if d_ins is not None else upload(torch, s, sc)
    want, want_k, want_m = kp.expect_chain(lrp, torch, s, sc, d_ins, gains, n, interp, mode, stream=stream, count=count)
    got, got_k, got_m = kp.run(lrp, torch, s, sc, d_ins, gains, n, interp, mode, stream=stream, count=count)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    what = f"{what}: gains {gains} n {n} interp {interp} mode {mode}"
    assert kp.same_output(s, got, want), f"{what}: the output"
    assert torch.equal(got_m, want_m), f"{what}: the coverage plane"
    if count:
        assert torch.equal(got_k, want_k), f"{what}: the count plane"
    else:
        assert got_k is None
    return got, got_k, got_m


def check_overlap(lrp, torch, s, sc, lo, hi, what, d_ins=None):
    d_ins = d_ins if d_ins is not None else upload(torch, s, sc)
    want = kp.expect_overlap(lrp, torch, s, sc, d_ins, lo, hi)
    got = kp.run_overlap(lrp, s, sc, d_ins, lo, hi)
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and tuple(got.shape) == (8, 8, 2) and got.is_cuda
    g, w = got.cpu().numpy(), want.cpu().numpy()
    assert (g == w).all(), f"{what}: {np.argwhere(g != w)[:4].tolist()} got {g[g != w][:4]} want {w[g != w][:4]}"
    return w


# ================================================================== compose: the rig
@pytest.mark.parametrize("fmt", list(kp.FORMATS))
@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_rig_cells(lrp, torch_cuda, out_name, fmt):
    """Every instantiation of four lanes: 5 target lenses x 3 samplers x {rgba8, half}, every mode, n = 1."""
    s, sc = kp.FORMATS[fmt], kp.rig_scene(lrp, out_name)
    d_ins = upload(torch_cuda, s, sc)
    for interp in (0, 1, 2):
        for mode in kp.MODES:
            _, k, m = check(lrp, torch_cuda, s, sc, None, 1, interp, mode, f"{out_name} {fmt}", d_ins)
    k, m = k.cpu().numpy(), m.cpu().numpy()
    assert (m == 0).any() and (k == 1).any() and (k >= 2).any()


@pytest.mark.parametrize("n", [2, 15])
def test_rig_n(lrp, torch_cuda, n):
    for out_name in ("eqr_part", "rect18"):
        for fmt in kp.FORMATS:
            s, sc = kp.FORMATS[fmt], kp.rig_scene(lrp, out_name)
            d_ins = upload(torch_cuda, s, sc)
            for interp, mode in ((2, FEATHER), (0, FIRST), (1, MEAN)):
                _, k, m = check(lrp, torch_cuda, s, sc, None, n, interp, mode, f"{out_name} {fmt}", d_ins)
            assert cam.discriminates(k.cpu().numpy(), m.cpu().numpy(), n)


@pytest.mark.parametrize("fmt", list(kp.FORMATS))
def test_gains_unit_gains_and_a_gain_of_zero(lrp, torch_cuda, fmt):
    torch = torch_cuda
    s, sc = kp.FORMATS[fmt], kp.rig_scene(lrp)
    d_ins = upload(torch, s, sc)
    for interp in (0, 1, 2):
        for mode in kp.MODES:
            check(lrp, torch, s, sc, kp.GAINS, 2, interp, mode, f"{fmt} GAINS", d_ins)
    for mode in kp.MODES:
        check(lrp, torch, s, sc, (0.0, 1.0, 0.5), 2, 1, mode, f"{fmt} a gain of 0.0", d_ins)
    # gains of 1.0f against the call without gains, and both against their chains
    for n, interp, mode in ((2, 0, FIRST), (2, 1, MEAN), (3, 2, FEATHER)):
        unit, uk, um = check(lrp, torch, s, sc, (1.0, 1.0, 1.0), n, interp, mode, f"{fmt} unit gains", d_ins)
        none, nk, nm = check(lrp, torch, s, sc, None, n, interp, mode, f"{fmt} no gains", d_ins)
        assert kp.same_output(s, unit, none) and torch.equal(uk, nk) and torch.equal(um, nm)
    with_gains = kp.run(lrp, torch, s, sc, d_ins, kp.GAINS, 2, 1, MEAN)[0]
    torch.cuda.synchronize()
    assert not kp.same_output(s, with_gains, unit)


# ================================================================== compose: channel set-ups
@pytest.mark.parametrize("name", list(kp.CHANNEL_SETUPS))
def test_channel_setups(lrp, torch_cuda, name):
    """C <= 4 and C > 4 lanes, the one-load-per-sample tap path, every output format, fills, post."""
    s, sc = kp.CHANNEL_SETUPS[name], kp.rig_scene(lrp)
    d_ins = upload(torch_cuda, s, sc)
    for n, interp, mode in ((1, 2, FEATHER), (2, 1, MEAN), (2, 0, FIRST)):
        check(lrp, torch_cuda, s, sc, kp.GAINS, n, interp, mode, name, d_ins)
        check(lrp, torch_cuda, s, sc, None, n, interp, mode, name, d_ins)


# ================================================================== compose: alignment and guard bytes
def _at_offset(torch, host, offset, guard=64, value=0xA5):
    """A device copy of `host` that starts `offset` samples behind an address aligned to four samples, between guard samples;
    returns (buffer, first sample, view shaped like host)."""
    t = pc.to_device(torch, host)
    buf = torch.full((guard + 8 + t.numel() + guard,), value if t.dtype == torch.uint8 else 0x5A5A, dtype=t.dtype, device="cuda")
    size = t.element_size()
    first = ((-buf.data_ptr() // size) % 4) + guard + offset
    view = buf[first:first + t.numel()].view(t.shape)
    assert (view.data_ptr() // size) % 4 == offset and view.is_contiguous()
    view.copy_(t)
    return buf, first, view


@pytest.mark.parametrize("fmt", list(kp.FORMATS))
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_bases_at_every_alignment_and_guard_bytes(lrp, torch_cuda, offset, fmt):
    """One launch whose four cameras sit 0, 1, 2 and 3 samples behind an aligned address: the tap path differs per camera.  The
    output and both planes lie `offset` samples / bytes behind one, between guards that stay intact."""
    torch = torch_cuda
    s, sc = kp.FORMATS[fmt], kp.eight_scene(lrp, 4)
    packed = kp.make_inputs(s, sc)
    aligned = upload(torch, s, sc, packed)
    moved = [_at_offset(torch, a, i)[2] for i, a in enumerate(packed)]
    ow, oh = sc["size"]
    for n, interp, mode in ((2, 2, FEATHER), (1, 1, MEAN), (2, 0, FIRST)):
        want, want_k, want_m = kp.expect_chain(lrp, torch, s, sc, aligned, kp.GAINS + (0.9,), n, interp, mode)
        out_buf, out_first, out = _at_offset(torch, pc.empty_output(kp.out_case(s, sc)), offset)
        plane_bufs = [_at_offset(torch, np.full((oh, ow), 0xEE, dtype=np.uint8), offset) for _ in range(2)]
        got, got_k, got_m = kp.run(lrp, torch, s, sc, moved, kp.GAINS + (0.9,), n, interp, mode, out=out, count=plane_bufs[0][2],
                                   coverage=plane_bufs[1][2])
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and got_k.data_ptr() == plane_bufs[0][2].data_ptr()
        assert kp.same_output(s, got, want) and torch.equal(got_k, want_k) and torch.equal(got_m, want_m), f"{fmt} offset {offset} interp {interp}"
        for buf, first, view in [(out_buf, out_first, out)] + plane_bufs:
            host, guard = buf.cpu().numpy(), (0xA5 if buf.dtype == torch.uint8 else 0x5A5A)
            assert (host[:first] == guard).all() and (host[first + view.numel():] == guard).all(), "guard samples written"


# ================================================================== compose: sizes and camera counts
@pytest.mark.parametrize("size", [(1, 1), (33, 9), (31, 8)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_partial_tiles(lrp, torch_cuda, size):
    for out_name in ("eqr_part", "rect18"):
        for fmt in kp.FORMATS:
            s, sc = kp.FORMATS[fmt], kp.rig_scene(lrp, out_name, size)
            d_ins = upload(torch_cuda, s, sc)
            for n, interp, mode in ((2, 2, FEATHER), (1, 1, FIRST)):
                check(lrp, torch_cuda, s, sc, kp.GAINS, n, interp, mode, f"{out_name} {fmt} {size}", d_ins)


def test_one_camera_eight_cameras_nine_refused(lrp, torch_cuda):
    torch = torch_cuda
    s = kp.FORMATS["rgba8"]
    # identity: every texel is its own pixel, and the 8-bit codes survive decode and encode
    sc = kp.identity_scene(lrp)
    packed = kp.make_inputs(s, sc)
    got, k, m = check(lrp, torch, s, sc, None, 1, 0, FIRST, "identity", upload(torch, s, sc, packed))
    assert np.array_equal(got.cpu().numpy(), packed[0]) and (k == 1).all() and (m == 1).all()
    for fmt in kp.FORMATS:
        s = kp.FORMATS[fmt]
        sc = kp.one_camera_scene(lrp)
        _, k, m = check(lrp, torch, s, sc, (1.3,), 2, 2, FEATHER, f"one camera {fmt}")
        assert (m.cpu().numpy() == 0).any() and (k.cpu().numpy() == 1).any()
        sc = kp.eight_scene(lrp)
        d_ins = upload(torch, s, sc)
        for n, interp, mode in ((2, 2, FEATHER), (1, 1, MEAN), (2, 0, FIRST)):
            _, k, m = check(lrp, torch, s, sc, tuple(0.6 + 0.1 * i for i in range(8)), n, interp, mode, f"eight {fmt}", d_ins)
        assert k.cpu().numpy().max() >= 3
    nine = kp.scene(sc["lout"], sc["size"], sc["cams"] + sc["cams"][:1], None)
    with pytest.raises(lrp.LrpError) as e:
        kp.run(lrp, torch, s, nine, d_ins + d_ins[:1], None, 1, 1, FIRST)
    assert e.value.status == lrp.Status.BAD_ARG
    with pytest.raises(lrp.LrpError) as e:
        kp.run_overlap(lrp, s, nine, d_ins + d_ins[:1], *kp.RANGE)
    assert e.value.status == lrp.Status.BAD_ARG


def test_no_rotations_side_stream_and_first_without_a_count_plane(lrp, torch_cuda):
    torch = torch_cuda
    for fmt in kp.FORMATS:
        s = kp.FORMATS[fmt]
        lout, cams, _ = cam.rig(lrp, "eqr_full")
        check(lrp, torch, s, kp.scene(lout, cam.OUT_SIZE, cams, None), kp.GAINS, 2, 1, MEAN, f"{fmt} no rotations")
        sc = kp.rig_scene(lrp)
        d_ins = upload(torch, s, sc)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            check(lrp, torch, s, sc, kp.GAINS, 2, 2, FEATHER, f"{fmt} side stream", d_ins, stream=side)
        # FIRST without a count plane leaves the camera loop early: the same image, the same coverage
        for interp in (0, 2):
            early, _, em = check(lrp, torch, s, sc, kp.GAINS, 2, interp, FIRST, f"{fmt} FIRST, no count plane", d_ins, count=False)
            full, _, fm = check(lrp, torch, s, sc, kp.GAINS, 2, interp, FIRST, f"{fmt} FIRST", d_ins)
            assert kp.same_output(s, early, full) and torch.equal(em, fm)
        out, k, m = kp.run(lrp, torch, s, sc, d_ins, None, 1, 1, MEAN, count=False, coverage=False)
        torch.cuda.synchronize()
        assert k is None and m is None and kp.same_output(s, out, kp.expect_chain(lrp, torch, s, sc, d_ins, None, 1, 1, MEAN)[0])


def test_geometry_cache_counters_unmoved(lrp, torch_cuda):
    s, sc = kp.FORMATS["rgba8"], kp.rig_scene(lrp)
    d_ins = upload(torch_cuda, s, sc)
    want = kp.expect_chain(lrp, torch_cuda, s, sc, d_ins, kp.GAINS, 1, 2, FEATHER)
    want_stats = kp.expect_overlap(lrp, torch_cuda, s, sc, d_ins, *kp.RANGE)
    lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        before = lrp.geometry_cache_stats()
        got = kp.run(lrp, torch_cuda, s, sc, d_ins, kp.GAINS, 1, 2, FEATHER)
        stats = kp.run_overlap(lrp, s, sc, d_ins, *kp.RANGE)
        torch_cuda.cuda.synchronize()
        assert lrp.geometry_cache_stats() == before, "a packed camera call moved the cache counters"
        assert kp.same_output(s, got[0], want[0]) and torch_cuda.equal(stats, want_stats)
    finally:
        lrp.release_cached_tables()


def planted_halves(sc, packed):
    """Besides the eight halves make_input plants somewhere: a 3 x 3 block of special halves at every camera's principal point,
    which the rig's scenes look at (-0, a denormal, +-inf, two NaNs, the largest half, -7.25, 1.0)."""
    special = np.array([0x8000, 0x0001, 0x7C00, 0x7E01, 0xFC00, 0x7BFF, 0xFE00, 0xC740, 0x3C00], dtype=np.uint16)
    for a, c in zip(packed, sc["cams"]):
        x0, y0 = int(round(c["cx"])) - 1, int(round(c["cy"])) - 1
        for j in range(9):
            a[y0 + j // 3, x0 + j % 3, :] = np.roll(special, j)[:a.shape[2]]
    return packed


@pytest.mark.parametrize("name", ["half", "half_c5"])
def test_planted_half_specials(lrp, torch_cuda, name):
    s = kp.FORMATS[name] if name in kp.FORMATS else kp.CHANNEL_SETUPS[name]
    sc = kp.rig_scene(lrp)
    d_ins = upload(torch_cuda, s, sc, planted_halves(sc, kp.make_inputs(s, sc)))
    nan_seen = False
    for interp in (0, 1, 2):
        for mode in kp.MODES:
            for gains in (kp.GAINS, (0.0, 1.0, 0.5), None):
                got, _, _ = check(lrp, torch_cuda, s, sc, gains, 2, interp, mode, f"planted {name}", d_ins)
                bits = got.cpu().numpy().view(np.uint16)
                nan_seen = nan_seen or bool((((bits & 0x7C00) == 0x7C00) & ((bits & 0x3FF) != 0)).any())
    assert nan_seen


def test_mid_size_frame(lrp, torch_cuda):
    """1040 x 513: 33 x 65 tiles, a partial last column and a last row of one line."""
    s, sc = kp.FORMATS["rgba8"], kp.rig_scene(lrp, "eqr_part", (1040, 513))
    d_ins = upload(torch_cuda, s, sc)
    check(lrp, torch_cuda, s, sc, kp.GAINS, 1, 1, FEATHER, "1040 x 513", d_ins)
    assert math.ceil(1040 / 32) * math.ceil(513 / 8) > 2048  # more tiles than the statistic's launch has workgroups
    want = check_overlap(lrp, torch_cuda, s, sc, *kp.RANGE, "1040 x 513", d_ins)
    assert want[0, 1, 0] > 10000


# ================================================================== the statistic
@pytest.mark.parametrize("fmt", list(kp.FORMATS))
@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_overlap_cells(lrp, torch_cuda, out_name, fmt):
    """Every instantiation: five target lenses x {8-bit, half}; all 128 words."""
    s = kp.FORMATS[fmt]
    lo, hi = kp.RANGE if fmt == "rgba8" else (0.6, 1.4)  # (halves are uniform in [0, 2))
    want = check_overlap(lrp, torch_cuda, s, kp.rig_scene(lrp, out_name), lo, hi, f"{out_name} {fmt}")
    assert all(want[i, j, 0] > 0 for i, j in ((0, 1), (0, 2), (1, 2))) and (want[3:] == 0).all() and (want[:, 3:] == 0).all()


def test_overlap_one_camera_and_eight(lrp, torch_cuda):
    for fmt in kp.FORMATS:
        s = kp.FORMATS[fmt]
        want = check_overlap(lrp, torch_cuda, s, kp.one_camera_scene(lrp), 0.1, 0.9, f"one camera {fmt}")
        assert want[0, 0, 0] > 0 and want[0, 0, 1] > 0 and np.count_nonzero(want) == 2
        want = check_overlap(lrp, torch_cuda, s, kp.eight_scene(lrp), 0.1, 0.9, f"eight cameras {fmt}")
        off = want[..., 0][~np.eye(8, dtype=bool)]
        assert (off == 0).any() and (off > 0).any() and (np.diagonal(want[..., 0]) > 0).all()


@pytest.mark.parametrize("size", [(1, 1), (33, 9), (31, 8)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_overlap_partial_tiles(lrp, torch_cuda, size):
    for out_name in ("eqr_part", "rect18"):
        for fmt in kp.FORMATS:
            want = check_overlap(lrp, torch_cuda, kp.FORMATS[fmt], kp.rig_scene(lrp, out_name, size), 0.0, 32768.0, f"{out_name} {fmt} {size}")
            assert 0 < want[..., 0].max() <= size[0] * size[1]


def test_overlap_prefilled_buffer_two_calls_and_side_stream(lrp, torch_cuda):
    torch = torch_cuda
    s, sc = kp.FORMATS["rgba8"], kp.rig_scene(lrp)
    d_ins = upload(torch, s, sc)
    want = kp.expect_overlap(lrp, torch, s, sc, d_ins, *kp.RANGE)
    buf = torch.full((8, 8, 2), -1, dtype=torch.int64, device="cuda")  # 0xFF bytes: every word is overwritten
    got = kp.run_overlap(lrp, s, sc, d_ins, *kp.RANGE, stats=buf)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and torch.equal(buf, want), "a buffer of 0xFF bytes"
    kp.run_overlap(lrp, s, sc, d_ins, 0.0, 1.0, stats=buf)  # two calls into one buffer, no synchronisation between them
    kp.run_overlap(lrp, s, sc, d_ins, *kp.RANGE, stats=buf)
    torch.cuda.synchronize()
    assert torch.equal(buf, want), "two calls into one buffer"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stats = kp.run_overlap(lrp, s, sc, d_ins, *kp.RANGE, stream=side)
    side.synchronize()
    assert torch.equal(stats, want), "side stream"


@pytest.mark.parametrize("name", ["gray8", "rgb8_pitch3", "in_packed_below_c", "in_packed_above_c", "half_c8", "out_packed_above_c"])
def test_overlap_channel_setups(lrp, torch_cuda, name):
    """C < 3: Y is channel 0; otherwise the luminance of channels 0-2, of which those behind in_pch are +0.0f."""
    s = kp.CHANNEL_SETUPS[name]
    lo, hi = (0.1, 0.6) if s["in_fmt"] == U8 else (0.4, 1.2)
    want = check_overlap(lrp, torch_cuda, s, kp.rig_scene(lrp), lo, hi, name)
    assert want[0, 1, 0] > 0


@pytest.mark.parametrize("fmt", list(kp.FORMATS))
def test_overlap_misaligned_bases(lrp, torch_cuda, fmt):
    torch = torch_cuda
    s, sc = kp.FORMATS[fmt], kp.eight_scene(lrp, 4)
    packed = kp.make_inputs(s, sc)
    want = kp.expect_overlap(lrp, torch, s, sc, upload(torch, s, sc, packed), 0.1, 0.9)
    for shift in (0, 1):
        moved = [_at_offset(torch, a, (i + shift) % 4)[2] for i, a in enumerate(packed)]
        got = kp.run_overlap(lrp, s, sc, moved, 0.1, 0.9)
        torch.cuda.synchronize()
        assert torch.equal(got, want), f"{fmt} shift {shift}"
    assert want[0, 1, 0].item() > 0


# ================================================================== end to end
def test_end_to_end_on_8_bit_frames(lrp, torch_cuda):
    """overlap_packed -> camera_gains -> compose_cameras_packed on the recovery scene (three frames of one world under exposures
    0.7, 1.0 and 1.4) as RGBA8, equal to the float chain: the table, the gains' bits, the bytes."""
    torch = torch_cuda
    s = kp.FORMATS["rgba8"]
    lout, cams, rots, srcs = gc.recovery_scene(lrp)
    sc = kp.scene(lout, cam.OUT_SIZE, cams, rots)
    d_ins = upload(torch, s, sc, [pc.encode_numpy(lrp, f, U8, 4, 0) for f in srcs])
    stats = kp.run_overlap(lrp, s, sc, d_ins, 0.02, 0.98)
    gains = lrp.camera_gains(stats, 3)
    want_stats = kp.expect_overlap(lrp, torch, s, sc, d_ins, 0.02, 0.98)
    want_gains = lrp.camera_gains(want_stats, 3)
    assert torch.equal(stats, want_stats) and all(stats[i, j, 0].item() > 0 for i, j in ((0, 1), (0, 2), (1, 2)))
    assert gains.dtype == np.float32 and (gains.view(np.uint32) == want_gains.view(np.uint32)).all() and gains[0] > 1.0 > gains[2]
    check(lrp, torch, s, sc, tuple(float(g) for g in gains), 2, 1, FEATHER, "end to end", d_ins)
