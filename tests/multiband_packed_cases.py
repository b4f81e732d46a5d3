"""The cases of the packed multi-band tests (include/lrp.h "multi-band blending, packed pixels"), shared by
tests/test_multiband_packed.py (CPU: the symbol, the error table, the mirror's refusals, and that every case discriminates) and
tests/test_gpu_multiband_packed.py (the call against the chain it is defined by, byte for byte on the output, the count plane and
the label plane).

The cases join two things the tests already have: the set-ups, the scenes, make_inputs and the numpy decode / encode of
tests/camera_packed_cases.py, and the scenes and the model of tests/multiband_cases.py / tests/multiband_model.py.

expect_chain() IS the definition: lrp_decode_pixels_device per camera -> lrp_compose_cameras_multiband_device ->
lrp_encode_pixels_device, with float32 temporaries of C channels — calls the library already has, never a second implementation.
cpu_chain() is the same chain without a GPU: numpy decode, the model of tests/multiband_model.py, numpy threshold encode."""
import numpy as np

import camera_cases as cam
import camera_packed_cases as kp
import multiband_cases as mb
import packed_cases as pc

F32, F16, U8 = kp.F32, kp.F16, kp.U8
NO_CAMERA = mb.NO_CAMERA
BANDS = mb.BANDS
GAINS = kp.GAINS
FORMATS = kp.FORMATS
# the set-ups of camera_packed_cases.CHANNEL_SETUPS a multi-band call takes: C <= 4
CHANNEL_SETUPS = {name: s for name, s in kp.CHANNEL_SETUPS.items() if s["C"] <= 4}
SIZES = [(1, 1), (31, 8), (33, 9), (5, 3), (270, 70)]


# ------------------------------------------------------------------ scenes (dicts of camera_packed_cases.scene)
def seam_scene(lrp, out_name="eqr_band", size=cam.OUT_SIZE):
    lout, cams, rots = mb.seam_rig(lrp, out_name, size)
    return kp.scene(lout, size, cams, rots)


def cut_scene(lrp, size=cam.OUT_SIZE):
    _, cams, rots = mb.seam_rig(lrp, "eqr_band", size)
    return kp.scene(mb.cut_lens(lrp), size, cams, rots)


def no_rotation_scene(lrp):
    lout, cams, _ = cam.rig(lrp, "eqr_full")
    return kp.scene(lout, cam.OUT_SIZE, cams, None)


def losers_scene(lrp):
    """Copies of cameras 0 .. 3 of the eight behind them: cameras that win nowhere."""
    sc = kp.eight_scene(lrp, 4)
    return kp.scene(sc["lout"], sc["size"], sc["cams"] + sc["cams"], sc["rots"] + sc["rots"])


def losers_inputs(s, sc):
    first = kp.make_inputs(s, kp.scene(sc["lout"], sc["size"], sc["cams"][:4], sc["rots"][:4]))
    return first + [a.copy() for a in first]


# ------------------------------------------------------------------ the chain on the CPU
def cpu_float(lrp, s, sc, packed_ins, gains, interp, bands):
    """tmp_out of the chain on the CPU — the float32 image (out_h, out_w, C) ahead of the encode — with the count and the label plane."""
    import multiband_model as mmodel

    srcs = [pc.decode_numpy(lrp, p, s["in_fmt"], s["C"]) for p in packed_ins]
    ow, oh = sc["size"]
    with np.errstate(all="ignore"):
        return mmodel.compose(sc["cams"], srcs, sc["lout"], ow, oh, interp, sc["rots"], bands, gains, s["post"])


def cpu_chain(lrp, s, sc, packed_ins, gains, interp, bands):
    """The packed output (out_h, out_w, out_pch), the count plane and the label plane of the chain, on the CPU."""
    img, count, label = cpu_float(lrp, s, sc, packed_ins, gains, interp, bands)
    return pc.encode_numpy(lrp, img, s["out_fmt"], s["out_pch"], s["fill"]), count, label


def nan_reaches(s, out, img):
    """Whether the planted NaNs show in a packed output `out` (numpy) of the float image `img` of cpu_float(); the text of what
    fails, or None.  The model's image has NaN samples and finite ones among the encoded channels; every NaN sample is code 255 (an
    8-bit output), a half NaN, or a float NaN; and among the finite ones some encode otherwise."""
    copy = min(s["C"], s["out_pch"])
    nan = np.isnan(img[..., :copy])
    if not nan.any() or nan.all():
        return f"{int(nan.sum())} of {nan.size} samples of the model's image are NaN"
    got = np.ascontiguousarray(out[..., :copy])
    if s["out_fmt"] == U8:
        is_nan = got == 255
    elif s["out_fmt"] == F16:
        bits = got.view(np.uint16)
        is_nan = ((bits & 0x7C00) == 0x7C00) & ((bits & 0x3FF) != 0)
    else:
        is_nan = np.isnan(got.view(np.float32))
    if not is_nan[nan].all():
        return "a NaN sample of the model's image is no NaN (8-bit: no 255) in the output"
    if is_nan[~nan].all():
        return "every finite sample encodes like a NaN"
    return None


def seam_pixels(label):
    """The number of 4-neighbour pairs that two different cameras win."""
    n = 0
    for la, lb in ((label[:, 1:], label[:, :-1]), (label[1:], label[:-1])):
        n += int(((la != lb) & (la != NO_CAMERA) & (lb != NO_CAMERA)).sum())
    return n


def discriminates(s, out, count, label, uncovered=True, cameras=2):
    """The conditions of a case; returns the text of what fails, or None.  `label` takes at least `cameras` camera values (two,
    or one for a one-camera scene) and NO_CAMERA where the scene has uncovered pixels; at least one seam pixel exists (two
    cameras); for an 8-bit output at least half of the covered pixels carry a colour code in 1 .. 254, and at least 32 distinct
    codes occur."""
    values = set(np.unique(label).tolist())
    if len(values - {NO_CAMERA}) < cameras:
        return f"label takes the camera values {sorted(values - {NO_CAMERA})}"
    if uncovered and NO_CAMERA not in values:
        return "no uncovered pixel"
    if ((label == NO_CAMERA) != (count == 0)).any():
        return "label and count disagree on what is covered"
    if cameras >= 2 and seam_pixels(label) < 1:
        return "no seam pixel"
    if s["out_fmt"] == U8:
        copy = min(s["C"], s["in_pch"], s["out_pch"], 3)
        codes = np.ascontiguousarray(out[..., :copy])[label != NO_CAMERA]
        inner = ((codes >= 1) & (codes <= 254)).any(axis=-1)
        if inner.sum() * 2 < inner.size:
            return f"{int(inner.sum())} of {inner.size} covered pixels carry a code in 1 .. 254"
        if np.unique(codes).size < 32:
            return f"{np.unique(codes).size} distinct codes"
    return None


# ------------------------------------------------------------------ the chain on the GPU: calls the library has
def aligned_scratch(lrp, torch, s, sc, bands, fill=None, extra=0):
    """(buffer, first, view): a uint8 CUDA buffer, and in it the scratch of the call, aligned to 256 bytes, with `extra` bytes
    behind it; fill: a byte value for the whole buffer."""
    need = lrp.multiband_scratch_bytes(sc["size"][0], sc["size"][1], s["C"], bands)
    buf = torch.empty((need + extra + 256,), dtype=torch.uint8, device="cuda") if fill is None else torch.full(
        (need + extra + 256,), fill, dtype=torch.uint8, device="cuda")
    first = (-buf.data_ptr()) % 256
    return buf, first, buf[first:first + need]


def expect_chain(lrp, torch, s, sc, d_ins, gains, interp, bands, stream=None):
    """The bytes lrp_compose_cameras_multiband_packed_device is defined to write: the output as a CUDA tensor (out_h, out_w,
    out_pch), prefilled like run()'s, and the count and the label plane (prefilled too)."""
    ow, oh = sc["size"]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        tmp_out = torch.full((oh, ow, s["C"]), -12345.0, dtype=torch.float32, device="cuda")
        out = pc.to_device(torch, pc.empty_output(kp.out_case(s, sc)))
    k, lab = kp.planes(torch, sc, stream)
    lrp.compose_cameras_multiband(kp.staged(lrp, torch, s, sc, d_ins, stream), kp.out_image(lrp, s, sc, tmp_out), interp, sc["rots"], bands,
                                  gains=gains, post=s["post"], count=k, label=lab, stream=stream)
    lrp.encode_pixels(tmp_out, out, s["out_fmt"], fill=s["fill"], stream=stream)
    return out, k, lab


def run(lrp, torch, s, sc, d_ins, gains, interp, bands, stream=None, out=None, count=True, label=True, scratch=None):
    """The call under test on the same inputs; the output tensor (prefilled like expect_chain's) and the two planes."""
    if out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            out = pc.to_device(torch, pc.empty_output(kp.out_case(s, sc)))
    k, lab = kp.planes(torch, sc, stream)
    count = k if count is True else (None if count is False else count)
    label = lab if label is True else (None if label is False else label)
    got = lrp.compose_cameras_multiband_packed(kp.cameras(lrp, sc), s["in_fmt"], d_ins, kp.out_image(lrp, s, sc), s["out_fmt"], out, s["fill"],
                                               interp, sc["rots"], bands, gains=gains, post=s["post"], count=count, label=label, scratch=scratch,
                                               stream=stream)
    return out, got[0], got[1]


def same_bytes(got, want):
    return np.array_equal(pc.as_bytes(got.cpu().numpy()), pc.as_bytes(want.cpu().numpy()))


# ------------------------------------------------------------------ the cases
def planted_halves(sc, packed):
    """Besides the eight halves make_input plants somewhere: a 3 x 3 block of special halves at every camera's principal point,
    which the rig's scenes look at (-0, a denormal, +-inf, two NaNs — one of them signalling —, the largest half, -7.25, 1.0)."""
    special = np.array([0x8000, 0x0001, 0x7C00, 0x7E01, 0xFC00, 0x7BFF, 0xFD00, 0xC740, 0x3C00], dtype=np.uint16)
    for a, c in zip(packed, sc["cams"]):
        x0, y0 = int(round(c["cx"])) - 1, int(round(c["cy"])) - 1
        for j in range(9):
            a[y0 + j // 3, x0 + j % 3, :] = np.roll(special, j)[:a.shape[2]]
    return packed


def case(group, name, s, scene, interp, bands, gains=None, inputs=None, uncovered=True, cameras=2, full=True, cpu=False):
    """scene: lrp -> scene; inputs: (s, scene) -> packed frames, default camera_packed_cases.make_inputs.  full: the case can hold every
    discrimination condition; false for the 1 x 1 target alone — one pixel has one label, so there are no two camera values and no
    pair of neighbours to be a seam, and its 3 colour samples cannot be 32 distinct codes — which is held to what it can show: a
    covered pixel.  cpu: the GPU test also compares against cpu_chain()."""
    return dict(group=group, name=name, s=s, scene=scene, interp=interp, bands=bands, gains=gains, inputs=inputs or kp.make_inputs,
                uncovered=uncovered, cameras=cameras, full=full, cpu=cpu)


HALF_TO_U8 = kp.setup(F16, U8)


def _cases():
    out = []
    for fmt, s in FORMATS.items():
        for interp in (0, 1, 2):
            out.append(case("cells", f"{fmt}-eqr_part-interp{interp}", s, lambda lrp: kp.rig_scene(lrp), interp, BANDS,
                            cpu=(fmt == "rgba8" and interp == 2)))
        for out_name in cam.OUT_LENSES:
            if out_name != "eqr_part":
                out.append(case("cells", f"{fmt}-{out_name}-interp1", s, lambda lrp, o=out_name: kp.rig_scene(lrp, o), 1, BANDS))
        for bands in (0, 1, 5, 8):
            out.append(case("bands", f"{fmt}-B{bands}", s, lambda lrp: kp.rig_scene(lrp), 2, bands, cpu=(fmt == "half" and bands == 5)))
    for size in SIZES:  # (the 18 mm view has no uncovered pixel, and neither has the partial panorama at 5 x 3)
        for f, o in (("rgba8", "eqr_part"), ("half", "rect18")):
            out.append(case("sizes", f"{f}-{o}-{size[0]}x{size[1]}", FORMATS[f], lambda lrp, o=o, z=size: kp.rig_scene(lrp, o, z), 1, BANDS,
                            full=size != (1, 1), uncovered=(o == "eqr_part" and size[0] * size[1] >= 31 * 8), cpu=(f == "rgba8" and size == (270, 70))))
    for fmt, s in FORMATS.items():
        out.append(case("wrap", f"{fmt}-seam", s, lambda lrp: seam_scene(lrp), 2, BANDS, uncovered=False, cpu=(fmt == "rgba8")))
        out.append(case("wrap", f"{fmt}-cut", s, lambda lrp: cut_scene(lrp), 2, BANDS, uncovered=False))
    out.append(case("wrap", "rgba8-seam-270x70", FORMATS["rgba8"], lambda lrp: seam_scene(lrp, size=(270, 70)), 1, 2, uncovered=False))
    for name, s in CHANNEL_SETUPS.items():
        out.append(case("channels", name, s, lambda lrp: kp.rig_scene(lrp), 2, BANDS, gains=GAINS, cpu=(name == "rgb8_pitch3")))
        out.append(case("channels", name + "-nearest", s, lambda lrp: kp.rig_scene(lrp), 0, 2))
    for fmt, s in FORMATS.items():
        out.append(case("cameras", f"{fmt}-one", s, lambda lrp: kp.one_camera_scene(lrp), 2, BANDS, cameras=1, cpu=(fmt == "half")))
        out.append(case("cameras", f"{fmt}-eight", s, lambda lrp: kp.eight_scene(lrp), 1, BANDS, cameras=6))
        out.append(case("cameras", f"{fmt}-losers", s, lambda lrp: losers_scene(lrp), 1, BANDS, inputs=losers_inputs, cameras=3))
        out.append(case("gains", f"{fmt}-no-rotations", s, lambda lrp: no_rotation_scene(lrp), 2, BANDS))
        for interp in (0, 1, 2):
            out.append(case("gains", f"{fmt}-gains-interp{interp}", s, lambda lrp: kp.rig_scene(lrp), interp, BANDS, gains=GAINS,
                            cpu=(fmt == "rgba8" and interp == 1)))
        out.append(case("gains", f"{fmt}-gain-zero", s, lambda lrp: kp.rig_scene(lrp), 1, BANDS, gains=(0.0, 1.0, 0.5)))
    planted = lambda s, sc: planted_halves(sc, kp.make_inputs(s, sc))
    # Into half: a gain of 0.0 meets the infinities (0 * inf is NaN).  Into 8-bit: a NaN or an infinity of level 0 reaches every
    # pixel within some 30 pixels of it through three bands, and a NaN is code 255 — the target is 320 x 96, so that more than half
    # of the covered pixels stay clear of the three blocks, and the gains keep halves of [0, 2) below 1.0.
    for name, s, size, some_gains in (("half", FORMATS["half"], cam.OUT_SIZE, (0.0, 1.0, 0.5)), ("half-to-u8", HALF_TO_U8, (320, 96), (0.25, 0.5, 0.5)),
                                      ("half-to-u8-post", kp.CHANNEL_SETUPS["f16_to_u8_tonemap"], (320, 96), (0.25, 0.5, 0.5))):
        for bands in (0, BANDS):
            for interp in (0, 1, 2):
                for gains in (None, some_gains):
                    out.append(case("specials", f"{name}-B{bands}-interp{interp}-{'gains' if gains else 'plain'}", s,
                                    lambda lrp, z=size: kp.rig_scene(lrp, "eqr_part", z), interp, bands, gains=gains, inputs=planted,
                                    cpu=(name == "half" and bands == BANDS and interp == 0 and not gains)))
    return out


CASES = _cases()


def group(name):
    return [c for c in CASES if c["group"] == name]


def case_id(c):
    return c["name"]
