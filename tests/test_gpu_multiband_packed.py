"""GPU: lrp_compose_cameras_multiband_packed_device (include/lrp.h "multi-band blending, packed pixels";
csrc/lrp_mb_packed_kernel.h) against the chain it is defined by, run on the GPU by the calls the library already has
(tests/multiband_packed_cases.py expect_chain): decode per camera -> compose_cameras_multiband -> encode.  Every comparison is
byte for byte — NaNs included: their signs and payloads are the chain's — on the output, the count plane and the label plane;
outputs and planes are prefilled on both sides.  One case of each group is also compared against the chain on the CPU
(cpu_chain; any NaN matches any NaN there, the model's NaNs carry the payloads of x86 arithmetic).
tests/test_multiband_packed.py shows on the CPU that the cases discriminate."""
import numpy as np
import pytest

import camera_cases as cam
import camera_gain_cases as gc
import camera_packed_cases as kp
import multiband_packed_cases as mp
import packed_cases as pc

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True  # (the tests set the cache themselves)
F32, F16, U8 = mp.F32, mp.F16, mp.U8


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


def upload(torch, packed):
    return [pc.to_device(torch, a) for a in packed]


def check(lrp, torch, s, sc, d_ins, gains, interp, bands, what, stream=None, **kw):
    """The call against the chain on the same device frames: the output and both planes, byte for byte."""
    want, want_k, want_l = mp.expect_chain(lrp, torch, s, sc, d_ins, gains, interp, bands, stream=stream)
    got, got_k, got_l = mp.run(lrp, torch, s, sc, d_ins, gains, interp, bands, stream=stream, **kw)
    (stream.synchronize if stream is not None else torch.cuda.synchronize)()
    what = f"{what}: gains {gains} interp {interp} B {bands}"
    assert mp.same_bytes(got, want), f"{what}: the output"
    assert torch.equal(got_k, want_k), f"{what}: the count plane"
    assert torch.equal(got_l, want_l), f"{what}: the label plane"
    return got, got_k, got_l


def check_case(lrp, torch, c):
    s, sc = c["s"], c["scene"](lrp)
    packed = c["inputs"](s, sc)
    got, k, lab = check(lrp, torch, s, sc, upload(torch, packed), c["gains"], c["interp"], c["bands"], c["name"])
    if c["cpu"]:
        out, count, label = mp.cpu_chain(lrp, s, sc, packed, c["gains"], c["interp"], c["bands"])
        assert pc.same_values(got.cpu().numpy(), out, s["out_fmt"]), f"{c['name']}: the output against the chain on the CPU"
        assert (k.cpu().numpy() == count).all() and (lab.cpu().numpy() == label).all(), f"{c['name']}: the planes against the chain on the CPU"
    return got, k, lab


@pytest.mark.parametrize("c", [c for g in ("cells", "bands", "sizes", "wrap", "channels", "cameras", "gains") for c in mp.group(g)], ids=mp.case_id)
def test_cases(lrp, torch_cuda, c):
    """Lenses and samplers; bands and sizes (270 x 70 at B = 3: 9 x 9 tiles of the new kernel, the last one partial in x and in
    y); the wrap and the clamp; channels and pitches; one camera, eight, cameras that win nowhere; no rotations, gains."""
    check_case(lrp, torch_cuda, c)


@pytest.mark.parametrize("name", ["half", "half-to-u8", "half-to-u8-post"])
def test_planted_half_specials(lrp, torch_cuda, name):
    """NaNs (a signalling one among them), infinities, -0 and a denormal at every camera's principal point, at B = 0 and B = 3:
    the bytes, and with them every NaN's sign, payload and quiet bit, are the chain's.  That the planted NaNs reach the output is
    read off the chain on the CPU: where its float image is NaN the output is (8-bit: code 255), and not everywhere else."""
    ran = 0
    for c in mp.group("specials"):
        if c["name"].rsplit("-B", 1)[0] == name:
            got, _, _ = check_case(lrp, torch_cuda, c)
            s, sc = c["s"], c["scene"](lrp)
            img, _, _ = mp.cpu_float(lrp, s, sc, c["inputs"](s, sc), c["gains"], c["interp"], c["bands"])
            why = mp.nan_reaches(s, got.cpu().numpy(), img)
            assert why is None, f"{c['name']}: {why}"
            ran += 1
    assert ran == 12


@pytest.mark.parametrize("fmt", list(mp.FORMATS))
def test_unit_gains_against_no_gains(lrp, torch_cuda, fmt):
    torch = torch_cuda
    s, sc = mp.FORMATS[fmt], kp.rig_scene(lrp)
    d_ins = upload(torch, kp.make_inputs(s, sc))
    for interp in (0, 2):
        unit = check(lrp, torch, s, sc, d_ins, (1.0, 1.0, 1.0), interp, mp.BANDS, f"{fmt} unit gains")
        none = check(lrp, torch, s, sc, d_ins, None, interp, mp.BANDS, f"{fmt} no gains")
        assert mp.same_bytes(unit[0], none[0]) and torch.equal(unit[1], none[1]) and torch.equal(unit[2], none[2])
    with_gains = mp.run(lrp, torch, s, sc, d_ins, mp.GAINS, 2, mp.BANDS)[0]
    torch.cuda.synchronize()
    assert not mp.same_bytes(with_gains, unit[0])


def test_nine_cameras_and_five_channels_refused(lrp, torch_cuda):
    torch = torch_cuda
    s, sc = mp.FORMATS["rgba8"], kp.eight_scene(lrp)
    d_ins = upload(torch, kp.make_inputs(s, sc))
    nine = kp.scene(sc["lout"], sc["size"], sc["cams"] + sc["cams"][:1], None)
    with pytest.raises(lrp.LrpError) as e:
        mp.run(lrp, torch, s, nine, d_ins + d_ins[:1], None, 1, 3)
    assert e.value.status == lrp.Status.BAD_ARG
    s5, sc = kp.CHANNEL_SETUPS["half_c5"], kp.rig_scene(lrp)
    with pytest.raises(lrp.LrpError) as e:
        mp.run(lrp, torch, s5, sc, upload(torch, kp.make_inputs(s5, sc)), None, 1, 3, scratch=torch.empty((1 << 20,), dtype=torch.uint8, device="cuda"))
    assert e.value.status == lrp.Status.CHANNELS


# ================================================================== alignment and guard bytes
def _at_offset(torch, host, offset, guard=64, value=0xA5):
    """A device copy of `host` that starts `offset` samples behind an address aligned to four samples, between guard samples;
    returns (buffer, first sample, view shaped like host)."""
    t = pc.to_device(torch, host)
    fill = {torch.uint8: value, torch.int16: 0x5A5A, torch.float32: -777.0}[t.dtype]
    buf = torch.full((guard + 8 + t.numel() + guard,), fill, dtype=t.dtype, device="cuda")
    size = t.element_size()
    first = ((-buf.data_ptr() // size) % 4) + guard + offset
    view = buf[first:first + t.numel()].view(t.shape)
    assert (view.data_ptr() // size) % 4 == offset and view.is_contiguous()
    view.copy_(t)
    return buf, first, view, fill


@pytest.mark.parametrize("name", ["rgba8", "half", "u8_to_f32_rgba"])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_bases_at_every_alignment_and_guard_bytes(lrp, torch_cuda, offset, name):
    """The output `offset` samples behind an address aligned to four samples — byte offsets 0-3 (8-bit), 0 / 2 / 4 / 6 (half),
    0 / 4 / 8 / 12 (float): one store per pixel at offset 0, one per sample otherwise — and both planes `offset` bytes behind one,
    between guards that stay intact.  The four frames sit 0, 1, 2 and 3 samples behind an aligned address (odd byte offsets among
    them)."""
    torch = torch_cuda
    s = mp.FORMATS[name] if name in mp.FORMATS else kp.setup(U8, F32)
    sc = kp.eight_scene(lrp, 4)
    packed = kp.make_inputs(s, sc)
    aligned = upload(torch, packed)
    moved = [_at_offset(torch, a, (i + offset) % 4)[2] for i, a in enumerate(packed)]
    ow, oh = sc["size"]
    gains = mp.GAINS + (0.9,)
    for interp, bands in ((2, 3), (0, 0)):
        want, want_k, want_l = mp.expect_chain(lrp, torch, s, sc, aligned, gains, interp, bands)
        out_buf, out_first, out, out_fill = _at_offset(torch, pc.empty_output(kp.out_case(s, sc)), offset)
        plane_bufs = [_at_offset(torch, np.full((oh, ow), 0xEE, dtype=np.uint8), offset) for _ in range(2)]
        got, got_k, got_l = mp.run(lrp, torch, s, sc, moved, gains, interp, bands, out=out, count=plane_bufs[0][2], label=plane_bufs[1][2])
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and got_k.data_ptr() == plane_bufs[0][2].data_ptr() and got_l.data_ptr() == plane_bufs[1][2].data_ptr()
        assert mp.same_bytes(got, want) and torch.equal(got_k, want_k) and torch.equal(got_l, want_l), f"{name} offset {offset} interp {interp}"
        for buf, first, view, fill in [(out_buf, out_first, out, out_fill)] + plane_bufs:
            host = buf.cpu().numpy()
            assert (host[:first] == fill).all() and (host[first + view.numel():] == fill).all(), "guard samples written"


# ================================================================== the scratch
def test_scratch(lrp, torch_cuda):
    torch = torch_cuda
    s, sc = mp.FORMATS["rgba8"], kp.rig_scene(lrp)
    d_ins = upload(torch, kp.make_inputs(s, sc))
    need = lrp.multiband_scratch_bytes(sc["size"][0], sc["size"][1], 4, 3)
    buf, first, scratch = mp.aligned_scratch(lrp, torch, s, sc, 3, fill=0xFF, extra=512)
    assert scratch.data_ptr() % 256 == 0 and scratch.numel() == need
    # pre-filled with 0xFF bytes (NaNs as floats); the planes in the scratch too (count=None, label=None)
    want3 = mp.expect_chain(lrp, torch, s, sc, d_ins, None, 2, 3)
    got, k, lab = mp.run(lrp, torch, s, sc, d_ins, None, 2, 3, scratch=scratch, count=False, label=False)
    torch.cuda.synchronize()
    assert k is None and lab is None and mp.same_bytes(got, want3[0]), "scratch of 0xFF bytes, no planes"
    assert (buf[first + need:].cpu().numpy() == 0xFF).all() and (buf[:first].cpu().numpy() == 0xFF).all(), "bytes behind the queried size written"
    # two different calls through one scratch buffer back to back, no synchronisation between them
    want1 = mp.expect_chain(lrp, torch, s, sc, d_ins, mp.GAINS, 1, 1)
    a = mp.run(lrp, torch, s, sc, d_ins, mp.GAINS, 1, 1, scratch=scratch)
    b = mp.run(lrp, torch, s, sc, d_ins, None, 2, 3, scratch=scratch)
    torch.cuda.synchronize()
    for got, want, what in ((a, want1, "first"), (b, want3, "second")):
        assert mp.same_bytes(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), f"{what} of two calls through one scratch"
    assert (buf[first + need:].cpu().numpy() == 0xFF).all()
    # one byte too small; misaligned by 128
    for bad in (buf[first:first + need - 1], buf[first + 128:first + 128 + need]):
        with pytest.raises(lrp.LrpError) as e:
            mp.run(lrp, torch, s, sc, d_ins, None, 2, 3, scratch=bad)
        assert e.value.status == lrp.Status.BAD_ARG and str(need) in str(e.value)


# ================================================================== the runtime
def test_side_stream_and_geometry_cache_counters(lrp, torch_cuda):
    torch = torch_cuda
    for fmt in mp.FORMATS:
        s, sc = mp.FORMATS[fmt], kp.rig_scene(lrp)
        d_ins = upload(torch, kp.make_inputs(s, sc))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            check(lrp, torch, s, sc, d_ins, mp.GAINS, 2, 3, f"{fmt} side stream", stream=side)
    want = mp.expect_chain(lrp, torch, s, sc, d_ins, mp.GAINS, 2, 3)
    lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        before = lrp.geometry_cache_stats()
        got = mp.run(lrp, torch, s, sc, d_ins, mp.GAINS, 2, 3)
        torch.cuda.synchronize()
        assert lrp.geometry_cache_stats() == before, "a packed multi-band call moved the cache counters"
        assert mp.same_bytes(got[0], want[0]) and torch.equal(got[2], want[2])
    finally:
        lrp.release_cached_tables()


# ================================================================== end to end
def test_chain_overlap_gains_multiband_on_8_bit_frames(lrp, torch_cuda):
    """camera_overlap_packed -> camera_gains -> compose_cameras_multiband_packed on the recovery scene (three frames of one world
    under exposures 0.7, 1.0 and 1.4) as RGBA8, equal to the same chain on decoded float frames, then encoded: the table, the
    gains' bits, the bytes."""
    torch = torch_cuda
    s = mp.FORMATS["rgba8"]
    lout, cams, rots, srcs = gc.recovery_scene(lrp)
    sc = kp.scene(lout, cam.OUT_SIZE, cams, rots)
    d_ins = upload(torch, [pc.encode_numpy(lrp, f, U8, 4, 0) for f in srcs])
    stats = kp.run_overlap(lrp, s, sc, d_ins, 0.02, 0.98)
    gains = lrp.camera_gains(stats, 3)
    want_stats = kp.expect_overlap(lrp, torch, s, sc, d_ins, 0.02, 0.98)
    want_gains = lrp.camera_gains(want_stats, 3)
    assert torch.equal(stats, want_stats) and all(stats[i, j, 0].item() > 0 for i, j in ((0, 1), (0, 2), (1, 2)))
    assert gains.dtype == np.float32 and (gains.view(np.uint32) == want_gains.view(np.uint32)).all() and gains[0] > 1.0 > gains[2]
    got, _, lab = check(lrp, torch, s, sc, d_ins, tuple(float(g) for g in gains), 1, 4, "end to end")
    plain = mp.run(lrp, torch, s, sc, d_ins, None, 1, 4)[0]
    torch.cuda.synchronize()
    assert not mp.same_bytes(got, plain) and mp.seam_pixels(lab.cpu().numpy()) > 0
