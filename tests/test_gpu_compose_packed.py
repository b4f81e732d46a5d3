"""-m gpu: lrp_compose_packed_device (include/lrp.h "compose, packed pixels"; csrc/lrp_compose_packed_kernel.h) — 8-bit and half
sources composed into a packed output by one launch — against the chain it is defined by, made of the three existing calls
(tests/compose_packed_cases.py expect_chain: decode_pixels per source -> compose -> encode_pixels): byte for byte on the output
AND on the count plane.  With an 8-bit source the comparison is strict for every output format; with a half source a NaN
matches a NaN (packed_cases.same_values).  Outputs are prefilled as packed_cases.empty_output does, on both sides.

All 30 cells x three samplers x three modes x {RGBA8, half}, the named compose cases under three format set-ups, the channel
set-ups, per-source alignment (one launch whose sources take different tap paths), output and count plane between guard bytes,
odd sizes, one and eight sources, tiny sources, no rotations, post, a side stream, the cache counters, planted half specials and
one mid-size frame."""
import numpy as np
import pytest

import compose_cases as cs
import compose_packed_cases as cp
import coverage_cases as cc
import packed_cases as pc

pytestmark = pytest.mark.gpu

F32, F16, U8 = cp.F32, cp.F16, cp.U8
RIG3 = cs.OVERLAP_CASES[0]  # three rectilinear cameras of two sizes into a panorama
FISH2 = cs.OVERLAP_CASES[1]  # two fisheyes 130 degrees apart
PART2 = cs.OVERLAP_CASES[2]  # two partial panoramas into an 18 mm view


@pytest.fixture(autouse=True)
def extensions_on(lrp, torch_cuda):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID | lrp.LENS_EXT_STEREOGRAPHIC)
    try:
        yield
    finally:
        lrp.lens_extensions(prev)


def check(lrp, torch, s, mode, interp, what, d_ins=None, rots="case", stream=None):
    """One call against the chain; returns k (numpy) and the output (numpy)."""
    if d_ins is None:
        d_ins = [pc.to_device(torch, a) for a in cp.make_inputs(s)]
    if rots == "case":
        rots = cp.rotations(lrp, s)
    want, want_k = cp.expect_chain(lrp, torch, s, d_ins, mode, interp, rots, stream=stream)
    got, got_k = cp.run(lrp, torch, s, d_ins, mode, interp, rots, stream=stream)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    label = f"{what}: {cs.MODE_NAMES[mode]} interp {interp}"
    assert got_k.dtype == torch.uint8 and tuple(got_k.shape) == tuple(want_k.shape)
    assert torch.equal(got_k, want_k), f"{label}: count plane"
    assert cp.same_output(s, got, want), f"{label}: output"
    return want_k.cpu().numpy(), got.cpu().numpy()


def sweep(lrp, torch, s, what, interps=(0, 1, 2)):
    d_ins = [pc.to_device(torch, a) for a in cp.make_inputs(s)]
    for interp in interps:
        for mode in cs.MODES:
            k, _ = check(lrp, torch, s, mode, interp, what, d_ins=d_ins)
    return k


CELLS = cc.cells()


@pytest.mark.parametrize("cell", CELLS, ids=[f"{o}<-{s}" for o, s, _ in CELLS])
def test_cells(lrp, torch_cuda, cell):
    case = cs.cell_case(*cell)
    for fmt in cp.CELL_FORMATS:
        k = sweep(lrp, torch_cuda, cp.setup(case, **cp.FORMATS[fmt]), f"{case['name']} {fmt}")
    assert (k >= 2).any() and (k == 1).any(), "a cell without overlap checks no accumulation"


@pytest.mark.parametrize("fmt", list(cp.FORMATS))
@pytest.mark.parametrize("case", cs.CASES, ids=[c["name"] for c in cs.CASES])
def test_cases(lrp, torch_cuda, case, fmt):
    k = sweep(lrp, torch_cuda, cp.setup(case, **cp.FORMATS[fmt]), f"{case['name']} {fmt}")
    if case is cs.CUBE:  # the seams, read off the count plane: the model's figures (tests/test_compose.py)
        assert int((k == 0).sum()) == cs.CUBE_SEAMS["k0"] and int((k >= 2).sum()) == cs.CUBE_SEAMS["k2"]
    else:
        assert min((k == 0).mean(), (k == 1).mean(), (k >= 2).mean()) >= 0.05


# Channel set-ups, two sources each.  C <= 4 runs the 4-lane kernels, C 5 and 8 the 8-lane ones.
CHANNEL_SETUPS = {
    "gray8": dict(in_fmt=U8, out_fmt=U8, C=1, in_pch=1, out_pch=1),
    "rgb8_pitch3": dict(in_fmt=U8, out_fmt=U8, C=3, in_pch=3, out_pch=3),
    "rgba8_c3_fill255": dict(in_fmt=U8, out_fmt=U8, C=3, in_pch=4, out_pch=4, fill=255),
    "half_c5": dict(in_fmt=F16, out_fmt=F16, C=5, in_pch=5, out_pch=5),
    "half_c8": dict(in_fmt=F16, out_fmt=F16, C=8, in_pch=8, out_pch=8),
    "u8_c8": dict(in_fmt=U8, out_fmt=U8, C=8, in_pch=8, out_pch=8),
    "in_packed_below_c": dict(in_fmt=U8, out_fmt=U8, C=4, in_pch=3, out_pch=4),  # channel 3 is a +0.0f tap
    "in_packed_above_c": dict(in_fmt=F16, out_fmt=F16, C=2, in_pch=4, out_pch=2),
    "in_packed_above_c_8_lanes": dict(in_fmt=U8, out_fmt=U8, C=5, in_pch=7, out_pch=5),
    "out_packed_below_c": dict(in_fmt=U8, out_fmt=U8, C=4, in_pch=4, out_pch=2),
    "out_packed_above_c": dict(in_fmt=F16, out_fmt=F16, C=2, in_pch=2, out_pch=6, fill=0x3C00),
    "out_packed_above_c_u8": dict(in_fmt=U8, out_fmt=U8, C=3, in_pch=3, out_pch=5, fill=0x7B),
    "u8_to_f16": dict(in_fmt=U8, out_fmt=F16, C=4),
    "u8_to_f32": dict(in_fmt=U8, out_fmt=F32, C=3, fill=0x3F800000),
    "u8_to_f32_pitch5": dict(in_fmt=U8, out_fmt=F32, C=3, in_pch=3, out_pch=5, fill=0x7FC00001),
    "f16_to_u8_tonemap": dict(in_fmt=F16, out_fmt=U8, C=4, post=cp.POST),
    "f16_to_f32": dict(in_fmt=F16, out_fmt=F32, C=4),
    "f16_c3_to_rgba8_tonemap": dict(in_fmt=F16, out_fmt=U8, C=3, in_pch=3, out_pch=4, fill=255, post=cp.POST),
}


@pytest.mark.parametrize("name", list(CHANNEL_SETUPS))
def test_channel_setups(lrp, torch_cuda, name):
    s = cp.setup(FISH2, **CHANNEL_SETUPS[name])
    d_ins = [pc.to_device(torch_cuda, a) for a in cp.make_inputs(s)]
    for mode, interp in ((cs.FIRST, 2), (cs.MEAN, 1), (cs.FEATHER, 0), (cs.FEATHER, 2)):
        k, got = check(lrp, torch_cuda, s, mode, interp, name, d_ins=d_ins)
        assert (k == 0).mean() >= 0.05 and (k >= 2).mean() >= 0.05
        if s["out_pch"] > s["C"]:  # the fill, looked at on the uncovered pixels too (and not only through the chain)
            fill = got.view(pc.NUMPY_TYPES[s["out_fmt"]])[..., s["C"]:]
            mask = {U8: 0xFF, F16: 0xFFFF, F32: 0xFFFFFFFF}[s["out_fmt"]]
            bits = fill.view(np.uint32) if s["out_fmt"] == F32 else fill
            assert (bits == (s["fill"] & mask)).all() and (bits[k == 0] == (s["fill"] & mask)).all(), f"{name}: fill"
        zero = got.view(np.uint32 if s["out_fmt"] == F32 else pc.NUMPY_TYPES[s["out_fmt"]])[..., :min(s["C"], s["out_pch"])][k == 0]
        assert (zero == 0).all(), f"{name}: a k == 0 pixel is +0.0f (code 0) in the first C channels"


def _guarded(torch, nbytes, offset, align=16, guard=64, value=0xA5):
    """A uint8 buffer with `nbytes` at `offset` bytes past an `align` boundary between `guard` bytes on either side."""
    assert guard % align == 0 and 0 <= offset < align
    buf = torch.full((align + guard + align + nbytes + guard,), value, dtype=torch.uint8, device="cuda")
    first = (-buf.data_ptr()) % align + guard + offset
    assert (buf.data_ptr() + first) % align == offset and first >= guard and first + nbytes + guard <= buf.numel()
    return buf, first


def _rig_three_sizes():
    return cs._case("rig3_sizes", "eqr_full", (96, 48), [("rect18", (64, 48), (0.0, 0.0, 0.0)), ("rect12", (48, 32), (40.0, 0.0, 0.0)), ("rect18", (56, 40), (80.0, 0.0, 0.0))])


@pytest.mark.parametrize("offsets", [(0, 1, 2), (1, 2, 0), (2, 0, 1)], ids=lambda o: "-".join(map(str, o)))
def test_per_source_alignment(lrp, torch_cuda, offsets):
    """Three RGBA8 sources of different sizes whose base pointers sit at different byte offsets: one takes the dword tap path,
    two the byte path, in ONE launch.  The chain reads aligned copies of the same bytes."""
    torch = torch_cuda
    s = cp.setup(_rig_three_sizes(), in_fmt=U8, out_fmt=U8)
    packed = cp.make_inputs(s)
    aligned = [pc.to_device(torch, a) for a in packed]
    views, keep = [], []
    for a, off in zip(packed, offsets):
        buf, first = _guarded(torch, a.size, off)
        buf[first:first + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        v = buf[first:first + a.size].view(a.shape)
        assert v.data_ptr() % 4 == off and v.is_contiguous()
        views.append(v)
        keep.append(buf)
    rots = cp.rotations(lrp, s)
    for mode in cs.MODES:
        for interp in (0, 1, 2):
            want, want_k = cp.expect_chain(lrp, torch, s, aligned, mode, interp, rots)
            got, got_k = cp.run(lrp, torch, s, views, mode, interp, rots)
            torch.cuda.synchronize()
            assert torch.equal(got_k, want_k) and cp.same_output(s, got, want), f"source offsets {offsets}: {cs.MODE_NAMES[mode]} interp {interp}"
    assert (want_k >= 2).any() and (want_k == 0).any()


@pytest.mark.parametrize("fmt", [U8, F16], ids=["u8", "f16"])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_output_alignment_and_guard_bytes(lrp, torch_cuda, offset, fmt):
    """The output base at byte offsets 0-3 (half: 0, 2, 4, 6 — a half pointer is 2-aligned) between 64 guard bytes that stay intact:
    offset 0 takes the one-store path, the others the per-sample path."""
    torch = torch_cuda
    for size in ((80, 48), (33, 9)):
        s = cp.setup(dict(RIG3, out_size=size), in_fmt=fmt, out_fmt=fmt)
        d_ins = [pc.to_device(torch, a) for a in cp.make_inputs(s)]
        rots = cp.rotations(lrp, s)
        sample = pc.SAMPLE_BYTES[fmt]
        nbytes = size[0] * size[1] * 4 * sample
        buf, first = _guarded(torch, nbytes, offset * sample)
        buf[first:first + nbytes] = 0x5A
        view = buf[first:first + nbytes].view(pc.torch_dtype(torch, fmt)).view(size[1], size[0], 4)
        assert view.data_ptr() % (4 * sample) == offset * sample
        want, want_k = cp.expect_chain(lrp, torch, s, d_ins, cs.FEATHER, 1, rots)
        got, got_k = cp.run(lrp, torch, s, d_ins, cs.FEATHER, 1, rots, out=view)
        torch.cuda.synchronize()
        assert got.data_ptr() == view.data_ptr()
        assert torch.equal(got_k, want_k) and cp.same_output(s, got, want), f"output offset {offset} {size}"
        host = buf.cpu().numpy()
        assert (host[:first] == 0xA5).all() and (host[first + nbytes:] == 0xA5).all(), "guard bytes written"


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_count_plane_alignment_and_guard_bytes(lrp, torch_cuda, offset):
    torch = torch_cuda
    for size in ((80, 48), (33, 9)):
        s = cp.setup(dict(RIG3, out_size=size), in_fmt=U8, out_fmt=U8)
        d_ins = [pc.to_device(torch, a) for a in cp.make_inputs(s)]
        rots = cp.rotations(lrp, s)
        n_px = size[0] * size[1]
        buf, first = _guarded(torch, n_px, offset, align=4)
        view = buf[first:first + n_px]
        assert view.data_ptr() % 4 == offset
        want, want_k = cp.expect_chain(lrp, torch, s, d_ins, cs.MEAN, 1, rots)
        got, got_k = cp.run(lrp, torch, s, d_ins, cs.MEAN, 1, rots, count=view)
        torch.cuda.synchronize()
        assert got_k.data_ptr() == view.data_ptr()
        host = buf.cpu().numpy()
        assert (host[first:first + n_px].reshape(size[1], size[0]) == want_k.cpu().numpy()).all() and int(want_k.max()) >= 2
        assert (host[:first] == 0xA5).all() and (host[first + n_px:] == 0xA5).all(), "guard bytes written"
        assert cp.same_output(s, got, want), "the image beside a misaligned plane"


@pytest.mark.parametrize("size", [(1, 1), (33, 9), (31, 8), (64, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(lrp, torch_cuda, size):
    """One pixel; a row that ends one lane into the second tile and a ninth row; a tile that is one lane short; four tiles."""
    for case, fmt in ((RIG3, "rgba8"), (PART2, "half")):
        s = cp.setup(dict(case, out_size=size), **cp.FORMATS[fmt])
        sweep(lrp, torch_cuda, s, f"{case['name']} {size} {fmt}", interps=(2, 1))


def test_one_source_and_eight_sources(lrp, torch_cuda):
    one = cs._case("one", "eqr_full", (96, 48), [("rect18", (64, 48), cc.GENERAL)])
    eight = cs._case("rig8", "eqr_full", (80, 48), [("rect18", (64 - 8 * (i % 2), 48), (35.0 * i, 10.0 * (i % 3) - 10.0, 0.0)) for i in range(8)])
    for fmt in ("rgba8", "half"):
        k = sweep(lrp, torch_cuda, cp.setup(one, **cp.FORMATS[fmt]), f"one source {fmt}", interps=(2, 0))
        assert k.max() == 1 and 0.05 < (k == 0).mean() < 0.95
        k = sweep(lrp, torch_cuda, cp.setup(eight, **cp.FORMATS[fmt]), f"eight sources {fmt}", interps=(2, 1))
        assert k.max() >= 3 and (k == 0).any()
    s = cp.setup(eight, **cp.FORMATS["rgba8"])
    d_ins = [pc.to_device(torch_cuda, a) for a in cp.make_inputs(s)]
    srcs, out_image = cp.images(lrp, s)
    with pytest.raises(lrp.LrpError) as e:  # nine: refused
        lrp.compose_packed(srcs + srcs[:1], U8, d_ins + d_ins[:1], out_image(None), U8, pc.to_device(torch_cuda, pc.empty_output(cp.out_case(s))), 0, 2)
    assert e.value.status == lrp.Status.BAD_ARG


@pytest.mark.parametrize("side", [1, 2])
def test_tiny_sources(lrp, torch_cuda, side):
    """Sources of 1 x 1 and 2 x 2 texels (every tap clamps to the same few texels): too few samples to discriminate, compared
    with the chain all the same."""
    for name, out in (("rect18", "eqr_full"), ("eqr_full", "rect18"), ("eqd_pi", "eqr_full")):
        case = cs._case(f"tiny{side}", out, (33, 9), [(name, (side, side), (0.0, 0.0, 0.0)), (name, (side, side), (25.0, 5.0, 0.0))])
        for fmt in ("rgba8", "half"):
            sweep(lrp, torch_cuda, cp.setup(case, **cp.FORMATS[fmt]), f"{side} x {side} {name} {fmt}")


def test_no_rotations(lrp, torch_cuda):
    """rotations == NULL: no source is rotated (and no multiplication happens)."""
    case = cs._case("unrotated", "eqr_full", (96, 48), [("rect18", (64, 48), None), ("rect12", (48, 32), None), ("rect35", (64, 48), None)])
    for fmt in ("rgba8", "half"):
        s = cp.setup(case, **cp.FORMATS[fmt])
        for mode in cs.MODES:
            k, _ = check(lrp, torch_cuda, s, mode, 2, f"no rotations {fmt}", rots=None)
        assert k.max() == 3 and (k == 0).any()


@pytest.mark.parametrize("post", [None, (2.0, 3.0)], ids=["plain", "tonemap"])
@pytest.mark.parametrize("channels", [1, 4])
def test_post_on_and_off(lrp, torch_cuda, channels, post):
    """The tonemap on the first min(C, 3) channels of the covered pixels only."""
    for in_fmt, out_fmt in ((U8, U8), (F16, F16), (F16, U8)):
        s = cp.setup(RIG3, in_fmt=in_fmt, out_fmt=out_fmt, C=channels, in_pch=channels, out_pch=channels, post=post)
        for mode, interp in ((cs.FIRST, 2), (cs.MEAN, 1), (cs.FEATHER, 0)):
            check(lrp, torch_cuda, s, mode, interp, f"C {channels} post {post}")


def test_side_stream(lrp, torch_cuda):
    torch = torch_cuda
    s = cp.setup(FISH2, **cp.FORMATS["rgba8"])
    d_ins = [pc.to_device(torch, a) for a in cp.make_inputs(s)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        check(lrp, torch, s, cs.FEATHER, 2, "side stream", d_ins=d_ins, stream=side)


def test_cache_counters_do_not_move(lrp, torch_cuda):
    torch = torch_cuda
    s = cp.setup(PART2, **cp.FORMATS["rgba8"])
    d_ins = [pc.to_device(torch, a) for a in cp.make_inputs(s)]
    rots = cp.rotations(lrp, s)
    prev = lrp.debug_set("geo_cache", 1)
    try:
        cp.run(lrp, torch, s, d_ins, cs.FIRST, 2, rots)  # (the first call on a device uploads the 8-bit tables)
        torch.cuda.synchronize()
        before = lrp.geometry_cache_stats()
        for mode in cs.MODES:
            cp.run(lrp, torch, s, d_ins, mode, 2, rots)
        torch.cuda.synchronize()
        assert lrp.geometry_cache_stats() == before, "a compose_packed call moved the cache counters"
    finally:
        lrp.debug_set("geo_cache", prev)


def test_planted_half_specials(lrp, torch_cuda):
    """Half sources carrying +-0, denormals, +-inf, a NaN and 65504 (packed_cases.PLANTED_HALVES), under all three modes and
    every output format; a NaN matches a NaN."""
    for out_fmt, post in ((F16, None), (F32, None), (U8, cp.POST)):
        s = cp.setup(RIG3, in_fmt=F16, out_fmt=out_fmt, post=post)
        packed = cp.make_inputs(s)
        for a in packed:
            assert set(pc.PLANTED_HALVES.tolist()) <= set(a.reshape(-1).tolist())
        d_ins = [pc.to_device(torch_cuda, a) for a in packed]
        for mode in cs.MODES:
            for interp in (1, 2):
                check(lrp, torch_cuda, s, mode, interp, f"planted -> {pc.FORMAT_NAMES[out_fmt]}", d_ins=d_ins)


def test_mid_size_frame(lrp, torch_cuda):
    """Two 512^2 RGBA8 equidistant fisheyes 130 degrees apart into 1024 x 512, bilinear FEATHER."""
    torch = torch_cuda
    case = cs._case("fisheye2_mid", "eqr_full", (1024, 512), [("eqd_pi", (512, 512), (0.0, 0.0, 0.0)), ("eqd_pi", (512, 512), (130.0, 0.0, 0.0))])
    s = cp.setup(case, **cp.FORMATS["rgba8"])
    d_ins = [pc.to_device(torch, a) for a in cp.make_inputs(s)]
    rots = cp.rotations(lrp, s)
    want, want_k = cp.expect_chain(lrp, torch, s, d_ins, cs.FEATHER, 1, rots)
    got, got_k = cp.run(lrp, torch, s, d_ins, cs.FEATHER, 1, rots)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got_k, want_k)
    assert float((want_k >= 2).float().mean()) > 0.05 and float((want_k == 0).float().mean()) > 0.05
    assert int(torch.unique(want).numel()) >= 200
