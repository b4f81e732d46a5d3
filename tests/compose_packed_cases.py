"""The cases of the packed compose tests (include/lrp.h "compose, packed pixels"), shared by tests/test_compose_packed.py (CPU:
the argument errors, and that every case discriminates) and tests/test_gpu_compose_packed.py (the one-launch call against the
chain it is defined by, byte for byte on the output and on the count plane).

The geometry is that of the compose tests (tests/compose_cases.py CASES and cell_case), the pixels those of the packed tests
(tests/packed_cases.py make_input, seed 100 + i for source i).  A set-up joins a compose case with the formats: C, the source
format and packed channels (one for all sources), the output format and packed channels, the fill and post.

expect_chain() IS the definition: lrp_decode_pixels_device per source -> lrp_compose_device -> lrp_encode_pixels_device with
float32 staging images of C channels — three calls the library already has, never a second implementation.  cpu_chain() is the
same chain without a GPU: numpy decode, the coverage model's render and coverage plane per source, compose_cases.expect, the
oracle's post_process on the covered pixels only, numpy threshold encode."""
import numpy as np

import cases
import compose_cases as cs
import packed_cases as pc

F32, F16, U8 = pc.F32, pc.F16, pc.U8
POST = pc.POST


def setup(case, in_fmt, out_fmt, C=4, in_pch=4, out_pch=4, fill=0, post=None):
    return dict(case=case, in_fmt=in_fmt, out_fmt=out_fmt, C=C, in_pch=in_pch, out_pch=out_pch, fill=fill, post=post)


# The format set-ups every compose case is run under.  (No half -> 8-bit without post: halves in [0, 2) clamp, and the cube case
# then has half of its covered samples at code 255.)
FORMATS = {
    "rgba8": dict(in_fmt=U8, out_fmt=U8),
    "half": dict(in_fmt=F16, out_fmt=F16),
    "half_to_rgba8_tonemap": dict(in_fmt=F16, out_fmt=U8, post=POST),
}
CELL_FORMATS = ("rgba8", "half")


def make_inputs(s):
    """The packed sources [(in_h, in_w, in_pch)]: packed_cases.make_input with seed 100 + i for source i."""
    return [pc.make_input(dict(in_size=size, in_fmt=s["in_fmt"], in_pch=s["in_pch"]), seed=100 + i) for i, (_, size, _) in enumerate(s["case"]["sources"])]


def out_case(s):
    """What packed_cases.empty_output reads of a case."""
    return dict(out_size=s["case"]["out_size"], out_pch=s["out_pch"], out_fmt=s["out_fmt"])


def rotations(lrp, s):
    return [cases.rotation(lrp, deg) for _, _, deg in s["case"]["sources"]]


# ------------------------------------------------------------------ the chain on the CPU
def cpu_parts(lrp, s, packed_ins, interp):
    """Per source: the model's render of the decoded source, its coverage plane and its feather weight."""
    import coverage_model as model

    lout, lins = cs.lenses(lrp, s["case"])
    ow, oh = s["case"]["out_size"]
    renders, planes, weights = [], [], []
    for lin, packed, (name, (w, h), deg) in zip(lins, packed_ins, s["case"]["sources"]):
        rot = cases.rotation(lrp, deg)
        src = pc.decode_numpy(lrp, packed, s["in_fmt"], s["C"])
        with np.errstate(all="ignore"):
            renders.append(model.reproject(lin, src, lout, ow, oh, 1, interp, rot))
        plane, sxy, _ = model.coverage(lin, w, h, lout, ow, oh, 1, rot, detail=True)
        planes.append(plane)
        weights.append(cs.feather_weight(sxy[:, :, 0, :], w, h, cs.wraps(name)))
    return renders, planes, weights


def cpu_chain(lrp, oracle, s, packed_ins, mode, interp, parts=None):
    """The packed output (out_h, out_w, out_pch) and k (out_h, out_w) of the chain, on the CPU."""
    renders, planes, weights = parts if parts is not None else cpu_parts(lrp, s, packed_ins, interp)
    img, k = cs.expect(mode, renders, planes, weights if mode == cs.FEATHER else None)
    if s["post"] is not None and (k > 0).any():  # the tonemap on the covered pixels only: a k == 0 pixel stays +0.0f
        covered = np.ascontiguousarray(img[k > 0]).reshape(-1, 1, s["C"])
        oracle.post_process(covered, *s["post"])
        img = img.copy()
        img[k > 0] = covered.reshape(-1, s["C"])
    return pc.encode_numpy(lrp, img, s["out_fmt"], s["out_pch"], s["fill"]), k


# ------------------------------------------------------------------ the chain on the GPU: three calls the library has
def images(lrp, s, datas=None):
    lout, lins = cs.lenses(lrp, s["case"])
    ow, oh = s["case"]["out_size"]
    srcs = [lrp.Image(lin, w, h, s["C"], None if datas is None else datas[i]) for i, (lin, (_, (w, h), _)) in enumerate(zip(lins, s["case"]["sources"]))]
    return srcs, (lambda data: lrp.Image(lout, ow, oh, s["C"], data))


def expect_chain(lrp, torch, s, d_ins, mode, interp, rots, stream=None):
    """The bytes lrp_compose_packed_device is defined to write — the output as a CUDA tensor (out_h, out_w, out_pch), prefilled
    like run()'s, and the count plane: decode_pixels per source -> compose -> encode_pixels with float32 staging images of C
    channels.  d_ins: the packed sources on the device."""
    ow, oh = s["case"]["out_size"]
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        tmps = [torch.empty((d.shape[0], d.shape[1], s["C"]), dtype=torch.float32, device="cuda") for d in d_ins]
        tmp_out = torch.full((oh, ow, s["C"]), -12345.0, dtype=torch.float32, device="cuda")
        out = pc.to_device(torch, pc.empty_output(out_case(s)))
        plane = torch.full((oh, ow), 0xEE, dtype=torch.uint8, device="cuda")
    for d, tmp in zip(d_ins, tmps):
        lrp.decode_pixels(d, s["in_fmt"], tmp, stream=stream)
    srcs, out_image = images(lrp, s, tmps)
    lrp.compose(srcs, out_image(tmp_out), interp, rots, mode, post=s["post"], count=plane, stream=stream)
    lrp.encode_pixels(tmp_out, out, s["out_fmt"], fill=s["fill"], stream=stream)
    return out, plane


def run(lrp, torch, s, d_ins, mode, interp, rots, stream=None, out=None, count=True):
    """The call under test on the same inputs; returns the output tensor (prefilled like expect_chain's) and the count plane."""
    if out is None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            out = pc.to_device(torch, pc.empty_output(out_case(s)))
    srcs, out_image = images(lrp, s)
    plane = lrp.compose_packed(srcs, s["in_fmt"], d_ins, out_image(None), s["out_fmt"], out, s["fill"], interp, rots, mode, post=s["post"],
                               count=count, stream=stream)
    return out, plane


def same_output(s, got, want):
    """Byte for byte with an 8-bit source (it cannot produce a NaN); with a half source a NaN matches a NaN
    (packed_cases.same_values)."""
    got, want = got.cpu().numpy(), want.cpu().numpy()
    if s["in_fmt"] == U8:
        return np.array_equal(pc.as_bytes(got), pc.as_bytes(want))
    return pc.same_values(got, want, s["out_fmt"])
