"""GPU: multi-band blending across a camera rig (include/lrp.h "multi-band blending across a camera rig";
csrc/lrp_multiband_kernel.h, csrc/lrp_multiband_label.hip) against the CPU model of tests/multiband_model.py, which
tests/test_multiband.py pins to the definition: the image byte for byte, any NaN matching any NaN, the count and the label plane
in every comparison."""
import numpy as np
import pytest

import camera_cases as cam
import camera_gain_cases as gc
import camera_gain_model as gmodel
import cases
import coverage_cases as cc
import multiband_cases as mb
import multiband_model as mmodel

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True  # (the tests set the cache themselves)


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


class Scene:
    """Cameras on the device and on the host: the frames, the rotations, the launch and the model's expectation."""

    def __init__(self, lrp, torch, lout, size, cams, rots, channels=4, seed=700, planted=False, host=None):
        self.lrp, self.torch, self.lout, self.cams, self.rots, self.C = lrp, torch, lout, cams, rots, channels
        self.ow, self.oh = size
        self.host = [np.ascontiguousarray(s) for s in (host if host is not None else cam.sources(cams, channels, seed, planted))]
        self.dev = [torch.from_numpy(s).cuda() for s in self.host]

    @classmethod
    def rig(cls, lrp, torch, out_name="eqr_part", size=cam.OUT_SIZE, **kw):
        lout, cams, rots = cam.rig(lrp, out_name, size)
        return cls(lrp, torch, lout, size, cams, rots, **kw)

    def cameras(self):
        return [cam.product(self.lrp, c, d) for c, d in zip(self.cams, self.dev)]

    def out_image(self, data=None):
        return self.lrp.Image(self.lout, self.ow, self.oh, self.C, data)

    def run(self, interp, bands, gains=None, post=None, count=True, label=True, scratch=None, stream=None, out=None):
        d = out if out is not None else self.torch.full((self.oh, self.ow, self.C), -1.0, dtype=self.torch.float32, device="cuda")
        planes = self.lrp.compose_cameras_multiband(self.cameras(), self.out_image(d), interp, self.rots, bands, gains=gains, post=post,
                                                    count=count, label=label, scratch=scratch, stream=stream)
        return d, planes

    def want(self, interp, bands, gains=None, post=None):
        return mmodel.compose(self.cams, self.host, self.lout, self.ow, self.oh, interp, self.rots, bands, gains, post)

    def compare(self, got, want, what):
        d, (count, label) = got
        cases.assert_same_bits(d.cpu().numpy(), want[0], what)
        assert (count.cpu().numpy().reshape(self.oh, self.ow) == want[1]).all(), f"{what}: count plane"
        assert (label.cpu().numpy().reshape(self.oh, self.ow) == want[2]).all(), f"{what}: label plane"

    def check(self, interp, bands, what, gains=None, post=None, **kw):
        got = self.run(interp, bands, gains=gains, post=post, **kw)
        self.torch.cuda.synchronize()
        want = self.want(interp, bands, gains, post)
        self.compare(got, want, f"{what}: interp {interp} B {bands} gains {gains} post {post}")
        return want


@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_cells(lrp, torch_cuda, out_name):
    """Every instantiation of the label kernel and of the level-0 layers: 5 target lenses x 3 samplers, B = 3."""
    scene = Scene.rig(lrp, torch_cuda, out_name)
    for interp in (0, 1, 2):
        img, count, label = scene.check(interp, mb.BANDS, out_name)
    assert (count == 0).any() and (count >= 2).any() and len(set(np.unique(label)) - {mb.NO_CAMERA}) >= 2


@pytest.mark.parametrize("bands", [0, 1, 5, 8])
def test_band_counts(lrp, torch_cuda, bands):
    Scene.rig(lrp, torch_cuda, "eqr_part").check(2, bands, "bands")


# 270 x 70 with B = 3: the levels are 270 x 70, 135 x 35, 68 x 18 and 34 x 9.  Every kernel works on 32 x 8 tiles of the level it
# writes: the label kernel, Laplacian-accumulate and collapse have 9 x 9 tiles at level 0, and reduce 5 x 5 at level 1 and 3 x 3
# at level 2; the last tile is partial in both axes at levels 0, 1 and 2 (270, 135, 68 are no multiples of 32; 70, 35, 18 none of 8).
@pytest.mark.parametrize("size,bands", [((1, 1), 3), ((31, 8), 3), ((33, 9), 3), ((5, 3), 3), ((270, 70), 3)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"B{v}")
def test_sizes(lrp, torch_cuda, size, bands):
    for out_name in ("eqr_part", "rect18"):
        Scene.rig(lrp, torch_cuda, out_name, size).check(1, bands, f"{out_name} {size}")


def test_wrap_across_the_seam_and_the_clamp_of_a_cut_lens(lrp, torch_cuda):
    """A full-turn target with the rig turned across the +-180 degree seam: X_k wraps, and a label boundary crosses the seam; the
    same lens cut short of a full turn clamps."""
    for size, bands in ((cam.OUT_SIZE, 3), ((33, 9), 3), ((270, 70), 2)):
        lout, cams, rots = mb.seam_rig(lrp, "eqr_band", size)
        scene = Scene(lrp, torch_cuda, lout, size, cams, rots)
        img, count, label = scene.check(2, bands, f"wrap {size}")
        assert (label[:, 0] != mb.NO_CAMERA).any() and (label[:, -1] != mb.NO_CAMERA).any()
        cut = Scene(lrp, torch_cuda, mb.cut_lens(lrp), size, cams, rots)
        clamped = cut.check(2, bands, f"cut {size}")
        assert (~cases.same_bits(clamped[0], img)).any()
    lout, cams, rots = mb.seam_rig(lrp, "eqr_full")
    Scene(lrp, torch_cuda, lout, cam.OUT_SIZE, cams, rots).check(1, 4, "eqr_full")


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_channels(lrp, torch_cuda, channels):
    scene = Scene.rig(lrp, torch_cuda, "eqr_part", channels=channels, seed=800 + channels)
    scene.check(2, 3, f"C {channels}")
    scene.check(0, 2, f"C {channels}", gains=gc.GAINS, post=(2.0, 3.0))


def test_five_channels_refused(lrp, torch_cuda):
    scene = Scene.rig(lrp, torch_cuda, "eqr_part", channels=5)
    with pytest.raises(lrp.LrpError) as e:
        scene.run(1, 3)
    assert e.value.status == lrp.Status.CHANNELS


def test_one_camera_then_eight_nine_refused(lrp, torch_cuda):
    torch = torch_cuda
    pano = cc.lens(lrp, "eqr_full", 80, 48)
    scene = Scene(lrp, torch, pano, (80, 48), [cam.resolve(lrp, cam.RIG[1])], [cases.rotation(lrp, cam.RIG_ROTATIONS[1])])
    img, count, label = scene.check(2, 3, "one camera")
    assert set(np.unique(label)) == {0, mb.NO_CAMERA}
    lout, cams, rots, srcs = gc.eight_scene(lrp)
    scene = Scene(lrp, torch, lout, (80, 48), cams, rots, host=srcs)
    img, count, label = scene.check(1, 3, "eight cameras")
    assert len(set(np.unique(label)) - {mb.NO_CAMERA}) >= 6 and count.max() >= 2
    # copies of cameras 0 .. 3 behind them: cameras that win nowhere
    copies = Scene(lrp, torch, lout, (80, 48), cams[:4] + cams[:4], rots[:4] + rots[:4], host=srcs[:4] + srcs[:4])
    img, count, label = copies.check(1, 3, "cameras that win nowhere")
    assert label[label != mb.NO_CAMERA].max() == 3
    with pytest.raises(lrp.LrpError) as e:  # nine: refused
        lrp.compose_cameras_multiband(scene.cameras() + scene.cameras()[:1], scene.out_image(torch.zeros((48, 80, 4), device="cuda")), 1)
    assert e.value.status == lrp.Status.BAD_ARG


def test_no_rotations(lrp, torch_cuda):
    lout, cams, _ = cam.rig(lrp, "eqr_full")
    img, count, label = Scene(lrp, torch_cuda, lout, cam.OUT_SIZE, cams, None).check(2, 3, "no rotations")
    assert (count >= 2).any()


def test_gains(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch)
    for interp in (0, 1, 2):
        scene.check(interp, 3, "gains", gains=gc.GAINS)
    scene.check(1, 3, "a gain of 0.0", gains=(0.0, 1.0, 0.5))
    planted = Scene.rig(lrp, torch, planted=True)
    planted.check(1, 2, "a gain of 0.0, planted", gains=(0.0, 1.0, 0.5))  # (0 * inf is NaN, in the model too)
    unit = scene.run(2, 3, gains=(1.0, 1.0, 1.0))
    none = scene.run(2, 3)
    torch.cuda.synchronize()
    cases.assert_same_bits(unit[0].cpu().numpy(), none[0].cpu().numpy(), "unit gains against gains=None")
    assert torch.equal(unit[1][0], none[1][0]) and torch.equal(unit[1][1], none[1][1])


def test_post_and_planted_specials(lrp, torch_cuda):
    scene = Scene.rig(lrp, torch_cuda)
    plain = scene.check(2, 3, "plain")
    toned = scene.check(2, 3, "post", post=(2.0, 3.0))
    assert (~cases.same_bits(plain[0][..., :3], toned[0][..., :3])).any()
    cases.assert_same_bits(plain[0][..., 3], toned[0][..., 3], "post leaves alpha")
    assert (toned[0][toned[2] == mb.NO_CAMERA] == 0).all()
    planted = Scene.rig(lrp, torch_cuda, planted=True)
    for interp in (0, 1, 2):
        want = planted.check(interp, 2, "planted", post=(2.0, 3.0) if interp == 1 else None)
    assert np.isnan(want[0]).any() and any(np.signbit(s[s == 0]).any() for s in planted.host)


def test_scratch(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch)
    need = lrp.multiband_scratch_bytes(scene.ow, scene.oh, 4, 3)
    guard = 512
    buf = torch.full((need + guard + 256,), 0xFF, dtype=torch.uint8, device="cuda")
    first = (-buf.data_ptr()) % 256
    scratch = buf[first:first + need]
    assert scratch.data_ptr() % 256 == 0
    # pre-filled with 0xFF bytes (NaNs as floats); the planes in the scratch too (count=None, label=None)
    want3 = scene.want(2, 3)
    d, planes = scene.run(2, 3, scratch=scratch, count=None, label=None)
    torch.cuda.synchronize()
    assert planes == (None, None)
    cases.assert_same_bits(d.cpu().numpy(), want3[0], "scratch of 0xFF bytes, no planes")
    assert (buf[first + need:].cpu().numpy() == 0xFF).all() and (buf[:first].cpu().numpy() == 0xFF).all(), "bytes behind the queried size written"
    # two different calls through one scratch buffer back to back, no synchronisation between them
    want1 = scene.want(1, 1, gc.GAINS)
    a = scene.run(1, 1, gains=gc.GAINS, scratch=scratch)
    b = scene.run(2, 3, scratch=scratch)
    torch.cuda.synchronize()
    scene.compare(a, want1, "first of two calls through one scratch")
    scene.compare(b, want3, "second of two calls through one scratch")
    assert (buf[first + need:].cpu().numpy() == 0xFF).all()
    # one byte too small; misaligned by 128
    for bad in (buf[first:first + need - 1], buf[first + 128:first + 128 + need]):
        with pytest.raises(lrp.LrpError) as e:
            scene.run(2, 3, scratch=bad)
        assert e.value.status == lrp.Status.BAD_ARG and str(need) in str(e.value)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_plane_alignment_and_guards(lrp, torch_cuda, offset):
    """count and label at byte offsets 0 to 3 between guard bytes; guard floats around the output, which starts at a float that
    is no multiple of 16 bytes for the odd offsets."""
    torch = torch_cuda
    size = (33, 9)
    scene = Scene.rig(lrp, torch, "eqr_part", size)
    n_px = size[0] * size[1]
    bufs, views = {}, {}
    for name in ("count", "label"):
        buf = torch.full((64 + 4 + n_px + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        first = (-buf.data_ptr()) % 4 + 64 + offset
        bufs[name], views[name] = (buf, first), buf[first:first + n_px]
        assert views[name].data_ptr() % 4 == offset
    pad = 16 + offset  # floats
    obuf = torch.full((pad + n_px * 4 + 16,), -777.0, dtype=torch.float32, device="cuda")
    out = obuf[pad:pad + n_px * 4].view(size[1], size[0], 4)
    d, got = scene.run(1, 3, count=views["count"], label=views["label"], out=out)
    torch.cuda.synchronize()
    want = scene.want(1, 3)
    for i, name in enumerate(("count", "label")):
        assert got[i].data_ptr() == views[name].data_ptr()
        buf, first = bufs[name]
        host = buf.cpu().numpy()
        assert (host[first:first + n_px].reshape(size[1], size[0]) == want[1 + i]).all(), f"{name} offset {offset}"
        assert (host[:first] == 0xA5).all() and (host[first + n_px:] == 0xA5).all(), "guard bytes written"
    host = obuf.cpu().numpy()
    cases.assert_same_bits(host[pad:pad + n_px * 4].reshape(size[1], size[0], 4), want[0], f"the image at float offset {pad}")
    assert (host[:pad] == -777.0).all() and (host[pad + n_px * 4:] == -777.0).all(), "guard floats written"


def test_side_stream_and_geometry_cache_counters(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch)
    want = scene.want(2, 3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = scene.run(2, 3, stream=side)
    side.synchronize()
    scene.compare(got, want, "side stream")
    lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        before = lrp.geometry_cache_stats()
        scene.check(2, 3, "cache on")
        assert lrp.geometry_cache_stats() == before, "a multi-band call moved the cache counters"
    finally:
        lrp.release_cached_tables()


def test_zero_bands_against_compose_cameras_on_the_device(lrp, torch_cuda):
    """B == 0: the pixel is +0.0f + the winner's one-camera render — compose_cameras itself, selected by label."""
    torch = torch_cuda
    for planted in (False, True):
        scene = Scene.rig(lrp, torch, planted=planted)
        for interp, gains in ((0, None), (1, None), (2, gc.GAINS)):
            d, (count, label) = scene.run(interp, 0, gains=gains)
            want = torch.zeros_like(d)
            for i, c in enumerate(scene.cameras()):
                one = torch.full_like(d, -1.0)
                lrp.compose_cameras([c], scene.out_image(one), 1, interp, [scene.rots[i]], 0, gains=None if gains is None else [gains[i]])
                want = torch.where((label == i)[..., None], one + 0.0, want)
            torch.cuda.synchronize()
            cases.assert_same_bits(d.cpu().numpy(), want.cpu().numpy(), f"B 0 planted {planted} interp {interp}")


def test_chain_overlap_gains_multiband(lrp, torch_cuda):
    """camera_overlap -> camera_gains -> compose_cameras_multiband equals the model's chain, on the recovery scene."""
    torch = torch_cuda
    lout, cams, rots, srcs = gc.recovery_scene(lrp)
    scene = Scene(lrp, torch, lout, cam.OUT_SIZE, cams, rots, host=srcs)
    stats = lrp.camera_overlap(scene.cameras(), scene.out_image(), rots, 0.02, 8.0)
    gains = lrp.camera_gains(stats, 3)
    want_gains = lrp.camera_gains(gmodel.overlap(cams, srcs, lout, scene.ow, scene.oh, rots, 0.02, 8.0), 3)
    assert (gains.view(np.uint32) == want_gains.view(np.uint32)).all() and gains[0] > 1.0 > gains[2]
    want = scene.check(1, 4, "chain", gains=gains)
    plain = scene.want(1, 4)
    assert mb.seam_step(want[0], want[2]) < mb.seam_step(plain[0], plain[2])
