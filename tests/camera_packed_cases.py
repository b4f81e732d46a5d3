"""The cases of the packed camera tests (include/lrp.h "calibrated cameras, packed pixels"), shared by tests/test_camera_packed.py
(CPU: the symbols, the error tables, the mirrors' refusals, and that every case discriminates) and
tests/test_gpu_camera_packed.py (the one-launch calls against the chains they are defined by: byte for byte on the output and
both planes, word for word on the overlap table).

The cases join three things the tests already have: the rig, eight() and IDENTITY of tests/camera_cases.py; the pixels of
tests/packed_cases.py (make_input, seed 100 + i for camera i); format set-ups in the style of tests/compose_packed_cases.py.

expect_chain() / expect_overlap() ARE the definitions: lrp_decode_pixels_device per camera -> lrp_compose_cameras(_gain)_device
-> lrp_encode_pixels_device, and decode -> lrp_camera_overlap_device, with float32 staging frames of C channels — calls the
library already has, never a second implementation.  cpu_chain() / cpu_overlap() are the same chains without a GPU: numpy
decode, the model of tests/camera_gain_model.py, numpy threshold encode.

A scene is a dict: lout (the target lens), size (out_w, out_h), cams (dicts of tests/camera_model.py), rots (matrices or None)."""
import numpy as np

import camera_cases as cam
import camera_gain_cases as gc
import cases
import coverage_cases as cc
import packed_cases as pc

F32, F16, U8 = pc.F32, pc.F16, pc.U8
POST = pc.POST
FIRST, MEAN, FEATHER = 0, 1, 2
MODES = (FIRST, MEAN, FEATHER)
GAINS = gc.GAINS
# lo, hi of the statistic's cases: chosen on the CPU model (tests/test_camera_packed.py test_overlap_cases_discriminate) so that
# on decoded 8-bit noise the three pairs of the rig have N_ij > 0 and the range excludes at least a quarter of what both cover
RANGE = (0.3, 0.8)


def setup(in_fmt, out_fmt, C=4, in_pch=4, out_pch=4, fill=0, post=None):
    return dict(in_fmt=in_fmt, out_fmt=out_fmt, C=C, in_pch=in_pch, out_pch=out_pch, fill=fill, post=post)


# The two set-ups the rig's sweeps run under.  (No half -> 8-bit without post: halves in [0, 2) clamp.)
FORMATS = {"rgba8": setup(U8, U8), "half": setup(F16, F16)}

CHANNEL_SETUPS = {
    "gray8": setup(U8, U8, C=1, in_pch=1, out_pch=1),
    "rgb8_pitch3": setup(U8, U8, C=3, in_pch=3, out_pch=3),  # the one-load-per-sample tap path
    "rgba8_c3_fill255": setup(U8, U8, C=3, fill=255),
    "half_c5": setup(F16, F16, C=5, in_pch=5, out_pch=5),
    "half_c8": setup(F16, F16, C=8, in_pch=8, out_pch=8),
    "in_packed_below_c": setup(U8, U8, in_pch=3),  # channel 3 is a +0.0f tap
    "in_packed_above_c": setup(F16, F16, C=2, out_pch=2),
    "out_packed_below_c": setup(U8, U8, out_pch=2),
    "out_packed_above_c": setup(F16, F16, C=2, in_pch=2, out_pch=6, fill=0x3C00),
    "u8_to_f16": setup(U8, F16),
    "u8_to_f32": setup(U8, F32, C=3, fill=0x3F800000),
    "f16_to_u8_tonemap": setup(F16, U8, post=POST),
}


# ------------------------------------------------------------------ scenes
def scene(lout, size, cams, rots):
    return dict(lout=lout, size=tuple(size), cams=cams, rots=rots)


def rig_scene(lrp, out_name="eqr_part", size=cam.OUT_SIZE):
    lout, cams, rots = cam.rig(lrp, out_name, size)
    return scene(lout, size, cams, rots)


def identity_scene(lrp):
    """One camera, every texel its own pixel."""
    return scene(cam.identity_lens(lrp), cam.IDENTITY["size"], [cam.IDENTITY], None)


def eight_scene(lrp, n=8):
    cams, rots = cam.eight(lrp)
    return scene(cc.lens(lrp, "eqr_full", 80, 48), (80, 48), cams[:n], rots[:n])


def one_camera_scene(lrp):
    """The rig's fisheye alone in a full panorama: pixels nobody sees, and no pixel two cameras see."""
    return scene(cc.lens(lrp, "eqr_full", 80, 48), (80, 48), [cam.resolve(lrp, cam.RIG[1])], [cases.rotation(lrp, cam.RIG_ROTATIONS[1])])


def make_inputs(s, sc, seed=100):
    """The packed frames [(height, width, in_pch)]: packed_cases.make_input with seed 100 + i for camera i."""
    return [pc.make_input(dict(in_size=c["size"], in_fmt=s["in_fmt"], in_pch=s["in_pch"]), seed=seed + i) for i, c in enumerate(sc["cams"])]


def out_case(s, sc):
    """What packed_cases.empty_output reads of a case."""
    return dict(out_size=sc["size"], out_pch=s["out_pch"], out_fmt=s["out_fmt"])


# ------------------------------------------------------------------ the chains on the CPU
def cpu_chain(lrp, s, sc, packed_ins, gains, n, interp, mode):
    """The packed output (out_h, out_w, out_pch), the count plane and the coverage plane of the chain, on the CPU.  gains None:
    gains of 1.0f (x * 1.0f == x)."""
    import camera_gain_model as gmodel

    srcs = [pc.decode_numpy(lrp, p, s["in_fmt"], s["C"]) for p in packed_ins]
    g = gains if gains is not None else (1.0,) * len(srcs)
    ow, oh = sc["size"]
    with np.errstate(all="ignore"):
        img, count, m = gmodel.compose(sc["cams"], srcs, g, sc["lout"], ow, oh, n, interp, sc["rots"], mode, s["post"])
    return pc.encode_numpy(lrp, img, s["out_fmt"], s["out_pch"], s["fill"]), count, m


def cpu_overlap(lrp, s, sc, packed_ins, lo, hi):
    import camera_gain_model as gmodel

    srcs = [pc.decode_numpy(lrp, p, s["in_fmt"], s["C"]) for p in packed_ins]
    ow, oh = sc["size"]
    return gmodel.overlap(sc["cams"], srcs, sc["lout"], ow, oh, sc["rots"], lo, hi)


def discriminates(s, out, count, m, n):
    """The geometry conditions and the code conditions of a compose case; returns the text of what fails, or None.  The codes
    are those of the channels that carry data: a channel behind in_pch is a +0.0f tap by definition, one code everywhere."""
    if n >= 2:
        if not cam.discriminates(count, m, n):
            return "the planes do not discriminate"
    elif not ((m == 0).any() and (count == 1).any() and (count >= 2).any()):
        return "no pixel with m == 0, count == 1 or count >= 2"
    copy = min(s["C"], s["in_pch"], s["out_pch"])
    codes = np.ascontiguousarray(out[..., :copy])[m > 0]
    codes = codes.view(np.uint32) if s["out_fmt"] == F32 else codes
    values, counts = np.unique(codes, return_counts=True)
    if values.size < 64:
        return f"{values.size} distinct codes among the covered samples"
    if counts.max() * 4 > codes.size:
        return f"code {values[counts.argmax()]} makes up {counts.max()} of {codes.size} covered samples"
    return None


# ------------------------------------------------------------------ the chains on the GPU: calls the library has
def staged(lrp, torch, s, sc, d_ins, stream=None):
    """The float32 frames of C channels the chain stages, as the package's cameras."""
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        tmps = [torch.empty((d.shape[0], d.shape[1], s["C"]), dtype=torch.float32, device="cuda") for d in d_ins]
    for d, tmp in zip(d_ins, tmps):
        lrp.decode_pixels(d, s["in_fmt"], tmp, stream=stream)
    return [cam.product(lrp, c, t) for c, t in zip(sc["cams"], tmps)]


def cameras(lrp, sc):
    return [cam.product(lrp, c) for c in sc["cams"]]


def out_image(lrp, s, sc, data=None):
    return lrp.Image(sc["lout"], sc["size"][0], sc["size"][1], s["C"], data)


def planes(torch, sc, stream=None):
    ow, oh = sc["size"]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        return (torch.full((oh, ow), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((oh, ow), 0xEE, dtype=torch.uint8, device="cuda"))


def expect_chain(lrp, torch, s, sc, d_ins, gains, n, interp, mode, stream=None, count=True):
    """The bytes lrp_compose_cameras_packed_device is defined to write: the output as a CUDA tensor (out_h, out_w, out_pch),
    prefilled like run()'s, and the two planes (prefilled too; count None when count is False)."""
    ow, oh = sc["size"]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        tmp_out = torch.full((oh, ow, s["C"]), -12345.0, dtype=torch.float32, device="cuda")
        out = pc.to_device(torch, pc.empty_output(out_case(s, sc)))
    k, m = planes(torch, sc, stream)
    lrp.compose_cameras(staged(lrp, torch, s, sc, d_ins, stream), out_image(lrp, s, sc, tmp_out), n, interp, sc["rots"], mode, post=s["post"],
                        count=k if count else None, coverage=m, stream=stream, gains=gains)
    lrp.encode_pixels(tmp_out, out, s["out_fmt"], fill=s["fill"], stream=stream)
    return out, (k if count else None), m


def run(lrp, torch, s, sc, d_ins, gains, n, interp, mode, stream=None, out=None, count=True, coverage=True):
    """The call under test on the same inputs; the output tensor (prefilled like expect_chain's) and the two planes."""
    if out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            out = pc.to_device(torch, pc.empty_output(out_case(s, sc)))
    k, m = planes(torch, sc, stream)
    count = k if count is True else (None if count is False else count)
    coverage = m if coverage is True else (None if coverage is False else coverage)
    got = lrp.compose_cameras_packed(cameras(lrp, sc), s["in_fmt"], d_ins, out_image(lrp, s, sc), s["out_fmt"], out, s["fill"], n, interp,
                                     sc["rots"], mode, post=s["post"], count=count, coverage=coverage, stream=stream, gains=gains)
    return out, got[0], got[1]


def expect_overlap(lrp, torch, s, sc, d_ins, lo, hi, stream=None):
    return lrp.camera_overlap(staged(lrp, torch, s, sc, d_ins, stream), out_image(lrp, s, sc), sc["rots"], lo, hi, stream=stream)


def run_overlap(lrp, s, sc, d_ins, lo, hi, **kw):
    return lrp.camera_overlap_packed(cameras(lrp, sc), s["in_fmt"], d_ins, out_image(lrp, s, sc), sc["rots"], lo, hi, **kw)


def same_output(s, got, want):
    """Byte for byte with an 8-bit source (it cannot produce a NaN); with a half source a NaN matches a NaN
    (packed_cases.same_values)."""
    got, want = got.cpu().numpy(), want.cpu().numpy()
    if s["in_fmt"] == U8:
        return np.array_equal(pc.as_bytes(got), pc.as_bytes(want))
    return pc.same_values(got, want, s["out_fmt"])
