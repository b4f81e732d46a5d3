"""The cases of the packed-pixel tests (include/lrp.h "packed pixels"), shared by tests/test_packed.py (CPU: the argument
errors, and that every case discriminates) and tests/test_gpu_packed.py (the one-launch call against the chain it is defined
by, byte for byte).

expect_chain() IS the definition: lrp_decode_pixels_device -> lrp_reproject_device -> lrp_encode_pixels_device with two float32
staging images of C channels — three calls the library already has, never a second implementation.  (Which kernel family
lrp_reproject_device renders with decides the sign and payload of a NaN sample, and nothing else: see expect_chain.)  cpu_chain() is the same
chain without a GPU: numpy decode with pixel_tables(), the oracle, numpy threshold encode.

A case: source lens name (tests/coverage_cases.py), source size, output lens name, output size, rotation in degrees or None,
C, source format and packed channels, output format and packed channels, fill, num_samples, interpolation, post or None."""
import numpy as np

import cases
import coverage_cases as cc

F32, F16, U8 = 0, 1, 2  # include/lrp.h lrp_pixel_format
FORMAT_NAMES = {F32: "f32", F16: "f16", U8: "u8"}
SAMPLE_BYTES = {F32: 4, F16: 2, U8: 1}
NUMPY_TYPES = {F32: np.float32, F16: np.uint16, U8: np.uint8}  # half samples travel as their bits
GENERAL = cc.GENERAL
POST = (2.0, 4.0)


def _case(name, inp, in_size, out, out_size, deg, C, in_fmt, in_pch, out_fmt, out_pch, fill=0, ns=1, interp=2, post=None):
    return dict(name=name, inp=inp, in_size=in_size, out=out, out_size=out_size, deg=deg, C=C, in_fmt=in_fmt, in_pch=in_pch,
                out_fmt=out_fmt, out_pch=out_pch, fill=fill, ns=ns, interp=interp, post=post)


_FISH_RECT = ("eqd_pi", (21, 13), "rect18", (33, 9))  # BASELINE configs[1] in small: a 180 degree fisheye into an 18 mm view
_PANO_FISH = ("eqr_full", (21, 13), "eqd_pi", (33, 9))  # configs[2]: a full panorama (wrapping) into a fisheye
_PANO_RECT = ("eqr_full", (21, 13), "rect18", (33, 9))

# The cases every test runs.  tests/test_packed.py checks on the CPU that each of them, and each case of cell_cases(),
# discriminates: the chain's result has at least 64 distinct codes and no code makes up more than half of its samples.
CASES = [
    # the channel set-ups
    _case("png_rgba8_c3_fill255", *_FISH_RECT, None, 3, U8, 4, U8, 4, fill=255),  # the PNG path: RGBA8, alpha dropped and written as 255
    _case("rgba8_c4", *_PANO_FISH, GENERAL, 4, U8, 4, U8, 4, interp=1),
    _case("gray8", *_PANO_RECT, GENERAL, 1, U8, 1, U8, 1),
    _case("rgb8_pitch3", *_FISH_RECT, None, 3, U8, 3, U8, 3, interp=1),
    _case("half_c5", *_PANO_RECT, GENERAL, 5, F16, 5, F16, 5),
    _case("half_c8", *_PANO_FISH, None, 8, F16, 8, F16, 8, interp=1),
    _case("half_rgba", *_FISH_RECT, GENERAL, 4, F16, 4, F16, 4),
    _case("in_packed_below_c", *_PANO_RECT, GENERAL, 4, U8, 3, U8, 4, interp=1),  # channel 3 is a +0.0f tap
    _case("in_packed_above_c", *_PANO_RECT, None, 2, F16, 4, F16, 2),
    _case("out_packed_below_c", *_PANO_RECT, GENERAL, 4, U8, 4, U8, 2),
    _case("out_packed_above_c", *_PANO_RECT, GENERAL, 2, F16, 2, F16, 6, fill=0x3C00),
    # every output format from both source formats
    _case("u8_to_f16", *_FISH_RECT, None, 4, U8, 4, F16, 4, interp=1),
    _case("u8_to_f32", *_FISH_RECT, None, 3, U8, 4, F32, 4, fill=0x3F800000),
    _case("u8_to_f32_pitch5", *_PANO_FISH, GENERAL, 3, U8, 3, F32, 5, fill=0x7FC00001, interp=0),
    _case("f16_to_u8", *_PANO_RECT, GENERAL, 4, F16, 4, U8, 4, post=POST),  # (the tonemap maps [0, 2) into [0, 1): without it half the samples clamp to 255)
    _case("f16_to_f32", *_PANO_FISH, GENERAL, 4, F16, 4, F32, 4, interp=1),
    _case("f16_c3_to_rgba8_tonemap", *_FISH_RECT, None, 3, F16, 3, U8, 4, fill=255, post=POST),
    # num_samples 1-3, tonemap on and off, the three samplers
    _case("ns2_bicubic_tonemap", *_PANO_RECT, GENERAL, 4, U8, 4, U8, 4, ns=2, post=POST),
    _case("ns3_bilinear", *_FISH_RECT, None, 4, F16, 4, F16, 4, ns=3, interp=1),
    _case("ns2_nearest_half_tonemap", *_PANO_FISH, GENERAL, 3, F16, 4, F16, 4, ns=2, interp=0, post=POST),
    _case("nearest_u8", *_PANO_FISH, GENERAL, 4, U8, 4, U8, 4, interp=0),
    _case("tonemap_c1", *_PANO_RECT, None, 1, F16, 1, F16, 1, post=POST),  # (the tonemap touches min(C, 3) channels)
    # outputs of 31 x 8 (one tile less a column) and 64 x 16 (four tiles); a 7 x 4 full-turn panorama with the seam in view
    _case("out_31x8", *_PANO_RECT[:3], (31, 8), GENERAL, 4, U8, 4, U8, 4),
    _case("out_64x16", *_FISH_RECT[:3], (64, 16), None, 4, F16, 4, U8, 4, interp=1, post=POST),
    _case("seam_7x4", "eqr_full", (7, 4), "rect18", (33, 9), (180.0, 0.0, 0.0), 4, U8, 4, F32, 4),
]

# Sources of 1 x 1 and 2 x 2 texels and the 1 x 1 output: too few samples for the bound above (a 1 x 1 source renders one
# value everywhere) — byte for byte against the chain on the GPU all the same.
TINY_CASES = [
    _case("src_1x1", "eqr_full", (1, 1), "rect18", (33, 9), GENERAL, 4, U8, 4, U8, 4),
    _case("src_2x2", "eqd_pi", (2, 2), "rect18", (33, 9), None, 3, F16, 3, F16, 4, fill=0x3C00, interp=1),
    _case("src_2x2_wrapping", "eqr_full", (2, 2), "eqd_pi", (33, 9), GENERAL, 4, U8, 4, U8, 4),
    _case("out_1x1", "eqr_full", (21, 13), "rect18", (1, 1), GENERAL, 4, U8, 4, U8, 4),
    _case("out_1x1_half", "eqd_pi", (21, 13), "rect18", (1, 1), None, 5, F16, 5, F32, 5, interp=1, ns=2),
]


# The rotations of the cell sweep: none, the general one, and the one of tests/coverage_cases.py that turns the view round (the
# fisheye targets look along +z, the others along -z: under it every cell sees the other side of a folding source).
CELL_ROTATIONS = [("norot", None), ("rot30", GENERAL), ("rot150", cc.CELL_ROTATIONS[1])]
# The one combination left out, because it cannot discriminate: the 18 mm view turned 150 degrees away from the partial
# panorama (+-1 rad of longitude) sees none of it, every pixel clamps to the panorama's nearest edge, and the 33 x 9 outputs
# hold the 13 texels of one edge column — 52 codes at most under the nearest sampler (49 on the CPU), fewer than the 64
# tests/test_packed.py asks for.  The cell itself
# is covered by the two other rotations.
CELL_LEFT_OUT = ("rect18", "eqr_part", "rot150")


def cell_cases():
    """The 30 cells of csrc/lrp_cells.h x 3 samplers x {8-bit, half} source, 33 x 9 out of 21 x 13, under CELL_ROTATIONS; RGBA in,
    RGBA out in the source's format.  tests/test_packed.py holds every one of them to the bound of CASES."""
    out = []
    for o, s, _size in cc.cells():
        for interp in (0, 1, 2):
            for fmt in (U8, F16):
                for rot, deg in CELL_ROTATIONS:
                    if (o, s, rot) != CELL_LEFT_OUT:
                        out.append(_case(f"{o}<-{s}/{interp}/{FORMAT_NAMES[fmt]}/{rot}", s, (21, 13), o, (33, 9), deg, 4, fmt, 4, fmt, 4, interp=interp))
    return out


def lenses(lrp, case):
    (iw, ih), (ow, oh) = case["in_size"], case["out_size"]
    return cc.lens(lrp, case["inp"], iw, ih), cc.lens(lrp, case["out"], ow, oh)


# the half texels every half source of 16 texels or more carries: +-0, denormals, +-inf, a NaN, the largest half
PLANTED_HALVES = np.array([0x0000, 0x8000, 0x0001, 0x83FF, 0x7C00, 0xFC00, 0x7E01, 0x7BFF], dtype=np.uint16)


def make_input(case, seed=1):
    """The packed source (in_h, in_w, in_pch): uniformly random bytes, or random halves in [0, 2) with PLANTED_HALVES."""
    iw, ih = case["in_size"]
    rng = np.random.default_rng(seed)
    if case["in_fmt"] == U8:
        return rng.integers(0, 256, size=(ih, iw, case["in_pch"]), dtype=np.uint8)
    a = (rng.random((ih, iw, case["in_pch"]), dtype=np.float32) * np.float32(2.0)).astype(np.float16).view(np.uint16)
    if iw * ih >= 16:
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=PLANTED_HALVES.size, replace=False)
        flat[idx] = PLANTED_HALVES
    return a


def empty_output(case, value=0x5A):
    ow, oh = case["out_size"]
    n = oh * ow * case["out_pch"] * SAMPLE_BYTES[case["out_fmt"]]
    return np.full(n, value, dtype=np.uint8).view(NUMPY_TYPES[case["out_fmt"]]).reshape(oh, ow, case["out_pch"])


def as_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# ------------------------------------------------------------------ the chain on the CPU
def decode_numpy(lrp, packed, fmt, C):
    """decode_kernel: the first min(packed channels, C) samples converted, +0.0f behind them."""
    h, w, pch = packed.shape
    out = np.zeros((h, w, C), dtype=np.float32)
    copy = min(pch, C)
    if fmt == U8:
        out[..., :copy] = lrp.pixel_tables()[0][packed[..., :copy]]
    else:
        out[..., :copy] = packed[..., :copy].view(np.float16).astype(np.float32)  # widening is exact
    return out


def encode_numpy(lrp, img, fmt, pch, fill):
    """encode_kernel: the first min(C, pch) channels converted, `fill` behind them."""
    h, w, C = img.shape
    copy = min(C, pch)
    v = np.ascontiguousarray(img[..., :copy], dtype=np.float32)
    if fmt == U8:
        thr = lrp.pixel_tables()[1]
        with np.errstate(invalid="ignore"):
            m = np.where(v < np.float32(1.0), v, np.float32(1.0))  # std::min(1.0f, v): NaN -> 1
            s = np.where(np.float32(0.0) < m, m, np.float32(0.0))  # std::max(0.0f, .): -0 -> +0
        out = np.full((h, w, pch), fill & 0xFF, dtype=np.uint8)
        out[..., :copy] = np.searchsorted(thr[1:], s, side="right").astype(np.uint8)  # thresholds 1..255 that s has reached
    elif fmt == F16:
        out = np.full((h, w, pch), fill & 0xFFFF, dtype=np.uint16)
        with np.errstate(over="ignore", invalid="ignore"):
            out[..., :copy] = v.astype(np.float16).view(np.uint16)  # round to nearest even, NaN payloads as include/lrp_half.h
    else:
        out = np.full((h, w, pch), fill & 0xFFFFFFFF, dtype=np.uint32)
        out[..., :copy] = v.view(np.uint32)
        out = out.view(np.float32)
    return out


EXTENSION_LENSES = ("eqs", "stg")  # lenses the oracle does not render


def cpu_chain(lrp, oracle, case, packed_in):
    """The chain on the CPU.  The render is the oracle's; with an equisolid or stereographic lens on either side, which the
    oracle does not have, it is the project's CPU model of those lenses (tests/coverage_model.py: the oracle's loop and samplers
    plus the two lenses)."""
    lin, lout = lenses(lrp, case)
    ow, oh = case["out_size"]
    src = decode_numpy(lrp, packed_in, case["in_fmt"], case["C"])
    if case["inp"] in EXTENSION_LENSES or case["out"] in EXTENSION_LENSES:
        import coverage_model

        img = coverage_model.reproject(lin, src, lout, ow, oh, case["ns"], case["interp"], cases.rotation(lrp, case["deg"]), post=case["post"])
    else:
        img = oracle.reproject(lin, src, lout, ow, oh, case["ns"], case["interp"], cases.rotation(lrp, case["deg"]))
        if case["post"] is not None:
            oracle.post_process(img, *case["post"])
    return encode_numpy(lrp, img, case["out_fmt"], case["out_pch"], case["fill"])


def same_values(got, want, fmt):
    """GPU against the CPU chain: the same bytes, except that any NaN matches any NaN (the oracle's NaNs carry the payloads of
    x86 arithmetic; tests/cases.py same_bits).  An 8-bit output has no NaN: byte for byte."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if fmt == U8:
        return np.array_equal(got, want)
    if fmt == F16:
        g, w = got.view(np.uint16), want.view(np.uint16)
        nan = lambda b: ((b & 0x7C00) == 0x7C00) & ((b & 0x3FF) != 0)  # noqa: E731
        return bool(((g == w) | (nan(g) & nan(w))).all())
    return bool(cases.same_bits(got.view(np.float32), want.view(np.float32)).all())


# ------------------------------------------------------------------ the chain on the GPU: three calls the library has
def torch_dtype(torch, fmt):
    return {F32: torch.float32, F16: torch.int16, U8: torch.uint8}[fmt]


def to_device(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def expect_chain(lrp, torch, case, d_in, stream=None, family=0):
    """The bytes lrp_reproject_packed_device is defined to write, as a CUDA tensor (out_h, out_w, out_pch): decode_pixels ->
    reproject -> encode_pixels with float32 staging images of C channels.  d_in: the packed source on the device.
    family: the kernel family lrp_reproject_device renders with (lrp_debug_kernel).  The families deliver the same bits except
    for the sign and payload of a NaN (tests/cases.py same_bits: the window kernel blends taps in another association than the
    samplers of csrc/lrp_device.h, and a NaN keeps the sign of the operand it came from).  The definition of include/lrp.h names
    family 0 — the one-pixel-per-lane kernel, whose samplers the packed kernel calls — and against that chain the comparison is
    byte for byte, NaNs included; None is the product's default family, compared with same_values()."""
    lin, lout = lenses(lrp, case)
    (iw, ih), (ow, oh), C = case["in_size"], case["out_size"], case["C"]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        tmp_in = torch.empty((ih, iw, C), dtype=torch.float32, device="cuda")
        tmp_out = torch.full((oh, ow, C), -12345.0, dtype=torch.float32, device="cuda")
        out = to_device(torch, empty_output(case))
    lrp.decode_pixels(d_in, case["in_fmt"], tmp_in, stream=stream)
    prev = lrp.debug_kernel(family) if family is not None else None
    try:
        lrp.reproject(lrp.Image(lin, iw, ih, C, tmp_in), lrp.Image(lout, ow, oh, C, tmp_out), case["ns"], case["interp"],
                      cases.rotation(lrp, case["deg"]), post=case["post"], stream=stream)
    finally:
        if prev is not None:
            lrp.debug_kernel(prev)
    lrp.encode_pixels(tmp_out, out, case["out_fmt"], fill=case["fill"], stream=stream)
    return out


def run_packed(lrp, torch, case, d_in, stream=None, out=None):
    """The call under test on the same inputs; returns the output tensor (prefilled like expect_chain's)."""
    lin, lout = lenses(lrp, case)
    (iw, ih), (ow, oh), C = case["in_size"], case["out_size"], case["C"]
    if out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            out = to_device(torch, empty_output(case))
    lrp.reproject_packed(lrp.Image(lin, iw, ih, C, None), case["in_fmt"], d_in, lrp.Image(lout, ow, oh, C, None), case["out_fmt"], out,
                         case["fill"], case["ns"], case["interp"], cases.rotation(lrp, case["deg"]), post=case["post"], stream=stream)
    return out


def tensor_bytes(t):
    return as_bytes(t.cpu().numpy())


def tensor_samples(t, fmt):
    a = t.cpu().numpy()
    return a.view(np.uint16) if fmt == F16 else a
