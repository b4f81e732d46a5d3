"""GPU: exposure matching across a camera rig (include/lrp.h "exposure matching across a camera rig"; csrc/lrp_camstat_kernel.h,
csrc/lrp_camgain_kernel.h) against the CPU model of tests/camera_gain_model.py, which tests/test_camera_gain.py pins to the
definition: the overlap table compared as integers, all 128 words; the gained compose byte for byte, any NaN matching any NaN,
both planes in every comparison."""
import math

import numpy as np
import pytest

import camera_cases as cam
import camera_gain_cases as gc
import camera_gain_model as gmodel
import camera_model as cmodel
import cases
import coverage_cases as cc

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True  # (the tests set the cache themselves)
FIRST, MEAN, FEATHER = 0, 1, 2
MODES = (FIRST, MEAN, FEATHER)


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
    """Cameras on the device and on the host: the frames, the rotations, the launches and the model's expectations."""

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

    # ---- the statistic
    def overlap(self, lo, hi, **kw):
        return self.lrp.camera_overlap(self.cameras(), self.out_image(), self.rots, lo, hi, **kw)

    def want_overlap(self, lo, hi):
        return gmodel.overlap(self.cams, self.host, self.lout, self.ow, self.oh, self.rots, lo, hi)

    def check_overlap(self, lo, hi, what):
        stats = self.overlap(lo, hi)
        self.torch.cuda.synchronize()
        assert stats.dtype == self.torch.int64 and tuple(stats.shape) == (8, 8, 2) and stats.is_cuda
        got, want = stats.cpu().numpy(), self.want_overlap(lo, hi)
        assert (got == want).all(), f"{what}: {np.argwhere(got != want)[:4].tolist()} got {got[got != want][:4]} want {want[got != want][:4]}"
        return want

    # ---- the gained compose
    def compose(self, gains, n, mode, interp, post=None, count=None, coverage=None, stream=None, fill=-1.0):
        d = self.torch.full((self.oh, self.ow, self.C), fill, dtype=self.torch.float32, device="cuda")
        planes = self.lrp.compose_cameras(self.cameras(), self.out_image(d), n, interp, self.rots, mode, post=post, count=count,
                                          coverage=coverage, stream=stream, gains=gains)
        return d, planes

    def check(self, gains, n, mode, interp, what, post=None):
        d, (count, coverage) = self.compose(gains, n, mode, interp, post=post, count=True, coverage=True)
        self.torch.cuda.synchronize()
        want, want_count, want_m = gmodel.compose(self.cams, self.host, gains, self.lout, self.ow, self.oh, n, interp, self.rots, mode, post)
        what = f"{what}: gains {tuple(gains)} n {n} mode {mode} interp {interp} post {post}"
        cases.assert_same_bits(d.cpu().numpy(), want, what)
        assert (count.cpu().numpy() == want_count).all(), f"{what}: count plane"
        assert (coverage.cpu().numpy() == want_m).all(), f"{what}: coverage plane"
        return want, want_count, want_m


# ================================================================== the statistic
@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_overlap_cells(lrp, torch_cuda, out_name):
    """Every instantiation: the five target lenses with the rig; all 128 words."""
    want = Scene.rig(lrp, torch_cuda, out_name).check_overlap(*gc.RANGE[out_name], out_name)
    assert sum(int(want[i, j, 0] > 0) for i, j in ((0, 1), (0, 2), (1, 2))) >= 2 and (want[3:] == 0).all() and (want[:, 3:] == 0).all()


def test_overlap_one_camera_then_eight_nine_refused(lrp, torch_cuda):
    torch = torch_cuda
    pano = cc.lens(lrp, "eqr_full", 80, 48)
    scene = Scene(lrp, torch, pano, (80, 48), [cam.resolve(lrp, cam.RIG[1])], [cases.rotation(lrp, cam.RIG_ROTATIONS[1])])
    want = scene.check_overlap(0.6, 0.9, "one camera")
    assert want[0, 0, 0] > 0 and want[0, 0, 1] > 0 and np.count_nonzero(want) == 2
    lout, cams, rots, srcs = gc.eight_scene(lrp)
    scene = Scene(lrp, torch, lout, (80, 48), cams, rots, host=srcs)
    want = scene.check_overlap(*gc.RANGE["eight"], "eight cameras")
    off = want[..., 0][~np.eye(8, dtype=bool)]
    assert (off == 0).any() and (off > 0).any() and (np.diagonal(want[..., 0]) > 0).all()
    with pytest.raises(lrp.LrpError) as e:  # nine: refused
        lrp.camera_overlap(scene.cameras() + scene.cameras()[:1], scene.out_image(), None)
    assert e.value.status == lrp.Status.BAD_ARG


def test_overlap_no_rotations(lrp, torch_cuda):
    lout, cams, _ = cam.rig(lrp, "eqr_full")
    want = Scene(lrp, torch_cuda, lout, cam.OUT_SIZE, cams, None).check_overlap(0.6, 0.9, "no rotations")
    assert want[0, 1, 0] > 0


def test_overlap_side_stream_prefilled_buffer_and_two_calls(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch)
    want = scene.want_overlap(0.6, 0.9)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stats = scene.overlap(0.6, 0.9, stream=side)
    side.synchronize()
    assert (stats.cpu().numpy() == want).all(), "side stream"
    # a buffer of 0xFF bytes: every word is overwritten, the zeroing runs on the stream ahead of the kernel
    buf = torch.full((8, 8, 2), -1, dtype=torch.int64, device="cuda")
    got = scene.overlap(0.6, 0.9, stats=buf)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr() and (buf.cpu().numpy() == want).all(), "a buffer of 0xFF bytes"
    # two calls in a row into one buffer, no synchronisation between them: the table of one call
    scene.overlap(0.3, 1.1, stats=buf)
    scene.overlap(0.6, 0.9, stats=buf)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == want).all(), "two calls into one buffer"


@pytest.mark.parametrize("size", [(1, 1), (33, 9), (31, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_overlap_partial_tiles(lrp, torch_cuda, size):
    """One pixel; a row that ends one lane into the second tile and a ninth row; a tile that is one lane short: lanes outside the
    image contribute nothing, and every lane reaches the workgroup's reduction."""
    for out_name in ("eqr_part", "rect18"):
        want = Scene.rig(lrp, torch_cuda, out_name, size).check_overlap(0.3, 1.2, f"{out_name} {size}")
        assert want[..., 0].max() <= size[0] * size[1] and want[..., 0].max() > 0


def test_overlap_workgroups_walk_several_tiles(lrp, torch_cuda):
    """More tiles than a launch has workgroups (2048): a workgroup walks several and adds once."""
    size = (1040, 513)
    assert math.ceil(size[0] / 32) * math.ceil(size[1] / 8) > 2048
    want = Scene.rig(lrp, torch_cuda, "eqr_part", size).check_overlap(0.6, 0.9, "1040 x 513")
    assert want[0, 1, 0] > 10000


def test_overlap_pixels_nobody_sees(lrp, torch_cuda):
    """An equisolid target whose frame reaches beyond its image circle: pixels with NaN rays, valid for no camera."""
    lout = lrp.LensInfo.equisolid(5.0, 36.0, 2 * math.pi, 80, 48)
    _, cams, rots = cam.rig(lrp, "eqs")
    ray = cmodel.detail(cams[0], lout, 80, 48, 1, rots[0])[0]
    assert np.isnan(ray).any(axis=-1).sum() > 1000
    want = Scene(lrp, torch_cuda, lout, (80, 48), cams, rots).check_overlap(0.6, 0.9, "NaN rays")
    assert want[0, 1, 0] > 0


def test_overlap_64_bit_carry(lrp, torch_cuda):
    """Frames of constant 32000.0: q = 32000 * 65536 > 2^30, so two pixels already overflow 32 bits."""
    lout, cams, rots = cam.rig(lrp, "eqr_part", (33, 9))
    host = [np.full((c["size"][1], c["size"][0], 3), 32000.0, dtype=np.float32) for c in cams]
    want = Scene(lrp, torch_cuda, lout, (33, 9), cams, rots, channels=3, host=host).check_overlap(0.0, 32768.0, "carry")
    assert want[..., 1].max() > 1 << 33 and (want[..., 1] == want[..., 0] * (32000 << 16)).all()


def test_overlap_planted_specials(lrp, torch_cuda):
    """Under lo = 0, hi = 32768: NaN, infinities, 3e38 and negatives are invalid; -0.0 and the denormal are valid with q = 0."""
    scene = Scene.rig(lrp, torch_cuda, planted=True)
    scene.check_overlap(0.0, 32768.0, "planted, 4 channels")
    scene = Scene.rig(lrp, torch_cuda, planted=True, channels=1)
    want = scene.check_overlap(0.0, 32768.0, "planted, 1 channel")
    assert any(np.signbit(s[s == 0]).any() for s in scene.host) and any(np.isnan(s).any() for s in scene.host)
    # one camera, identity geometry, one channel: every texel is its own pixel, Y = the texel
    # (the valid values first: at integer coordinates the bilinear sample is texel + 0 * neighbour, NaN beside an infinity)
    frame, q = gc.special_frame()
    ident = Scene(lrp, torch_cuda, cam.identity_lens(lrp), (64, 32), [cam.IDENTITY], None, channels=1, host=[frame])
    want = ident.check_overlap(0.0, 32768.0, "specials, identity")
    assert want[0, 0, 0] == 32 * 6 * len(q) and want[0, 0, 1] == 32 * 6 * sum(q)


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 11])
def test_overlap_channel_counts(lrp, torch_cuda, channels):
    """C < 3: Y is channel 0; otherwise the luminance of channels 0-2, whatever lies behind them."""
    Scene.rig(lrp, torch_cuda, "eqr_part", channels=channels, seed=800 + channels).check_overlap(0.6, 0.9, f"C {channels}")


def test_geometry_cache_counters_unmoved(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch)
    lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        before = lrp.geometry_cache_stats()
        scene.check_overlap(0.6, 0.9, "cache on")
        scene.check(gc.GAINS, 2, FEATHER, 2, "cache on")
        assert lrp.geometry_cache_stats() == before, "an exposure-matching call moved the cache counters"
    finally:
        lrp.release_cached_tables()


# ================================================================== the gained compose
@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_gain_cells(lrp, torch_cuda, out_name):
    """Every instantiation: 5 target lenses x 3 samplers, every mode, n 2, the gains 0.7, 1.0, 1.6."""
    scene = Scene.rig(lrp, torch_cuda, out_name)
    for interp in (0, 1, 2):
        for mode in MODES:
            want, count, m = scene.check(gc.GAINS, 2, mode, interp, out_name)
    assert (m == 0).any() and ((m > 0) & (m < 4)).any() and (m == 4).any() and (count >= 2).any()
    # FIRST without a count plane leaves the source loop early: the same image, the same coverage
    d, (none, coverage) = scene.compose(gc.GAINS, 2, FIRST, 2, coverage=True)
    torch_cuda.cuda.synchronize()
    want = gmodel.compose(scene.cams, scene.host, gc.GAINS, scene.lout, scene.ow, scene.oh, 2, 2, scene.rots, FIRST)
    assert none is None and (coverage.cpu().numpy() == want[2]).all()
    cases.assert_same_bits(d.cpu().numpy(), want[0], f"{out_name}: FIRST without a count plane")


@pytest.mark.parametrize("n", [1, 15])
def test_gain_n(lrp, torch_cuda, n):
    scene = Scene.rig(lrp, torch_cuda, "eqr_part")
    for interp, mode in ((2, FEATHER), (0, FIRST), (1, MEAN)):
        scene.check(gc.GAINS, n, mode, interp, "n")


@pytest.mark.parametrize("post", [None, (2.0, 3.0)], ids=["plain", "tonemap"])
@pytest.mark.parametrize("channels", [1, 2, 3, 4, 5, 8, 9, 11])
def test_gain_channels_and_post(lrp, torch_cuda, channels, post):
    """The gain on the first min(C, 3) channels of the first group of 8 only; 9, 11: the second group goes through the plain
    kernel."""
    scene = Scene.rig(lrp, torch_cuda, "eqr_part", channels=channels, seed=800 + channels)
    for n, mode, interp in ((2, FIRST, 2), (2, MEAN, 1), (2, FEATHER, 0)):
        scene.check(gc.GAINS, n, mode, interp, f"C {channels}", post=post)
    if post is None:  # channels beyond the colour are those of compose_cameras itself
        d, _ = scene.compose(gc.GAINS, 2, FEATHER, 1)
        plain, _ = scene.compose(None, 2, FEATHER, 1)
        torch_cuda.cuda.synchronize()
        cases.assert_same_bits(d.cpu().numpy()[..., 3:], plain.cpu().numpy()[..., 3:], f"C {channels}: beyond the colour")
        assert (~cases.same_bits(d.cpu().numpy()[..., :3], plain.cpu().numpy()[..., :3])).any()


def test_gain_zero_and_unit_gains(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch, planted=True)
    for mode in MODES:
        scene.check((0.0, 1.0, 0.5), 2, mode, 1, "a gain of 0.0")  # (0 * inf is NaN, in the model too)
    scene = Scene.rig(lrp, torch)
    want, _, _ = scene.check((0.0, 0.0, 0.0), 2, MEAN, 2, "all gains 0.0")
    assert (want[..., :3] == 0).all() and (want[..., 3] != 0).any()
    # gains of 1.0f against the output of compose_cameras itself, byte for byte, planted specials included
    for planted in (False, True):
        scene = Scene.rig(lrp, torch, planted=planted)
        for n, mode, interp, post in ((2, FIRST, 0, None), (2, MEAN, 1, None), (3, FEATHER, 2, None), (2, FEATHER, 1, (2.0, 3.0))):
            d, (count, m) = scene.compose((1.0, 1.0, 1.0), n, mode, interp, post=post, count=True, coverage=True)
            p, (pcount, pm) = scene.compose(None, n, mode, interp, post=post, count=True, coverage=True)
            torch.cuda.synchronize()
            cases.assert_same_bits(d.cpu().numpy(), p.cpu().numpy(), f"unit gains, planted {planted}, n {n} mode {mode} interp {interp}")
            assert torch.equal(count, pcount) and torch.equal(m, pm)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_gain_plane_alignment_and_guard_bytes(lrp, torch_cuda, offset):
    torch = torch_cuda
    size = (33, 9)
    scene = Scene.rig(lrp, torch, "eqr_part", size)
    n_px = size[0] * size[1]
    bufs, views = {}, {}
    for name in ("count", "coverage"):
        buf = torch.full((64 + 4 + n_px + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        first = (-buf.data_ptr()) % 4 + 64 + offset
        bufs[name], views[name] = (buf, first), buf[first:first + n_px]
        assert views[name].data_ptr() % 4 == offset
    d, got = scene.compose(gc.GAINS, 3, MEAN, 1, count=views["count"], coverage=views["coverage"])
    torch.cuda.synchronize()
    want, want_count, want_m = gmodel.compose(scene.cams, scene.host, gc.GAINS, scene.lout, 33, 9, 3, 1, scene.rots, MEAN)
    for i, (name, plane) in enumerate((("count", want_count), ("coverage", want_m))):
        assert got[i].data_ptr() == views[name].data_ptr()
        buf, first = bufs[name]
        host = buf.cpu().numpy()
        assert (host[first:first + n_px].reshape(size[1], size[0]) == plane).all(), f"{name} offset {offset}"
        assert (host[:first] == 0xA5).all() and (host[first + n_px:] == 0xA5).all(), "guard bytes written"
    cases.assert_same_bits(d.cpu().numpy(), want, "the image beside misaligned planes")


# ================================================================== end to end
def test_end_to_end_on_the_device(lrp, torch_cuda):
    """camera_overlap -> camera_gains -> compose_cameras(gains=...) equals the model's chain: three frames of one world under
    exposures 0.7, 1.0 and 1.4."""
    torch = torch_cuda
    lout, cams, rots, srcs = gc.recovery_scene(lrp)
    scene = Scene(lrp, torch, lout, cam.OUT_SIZE, cams, rots, host=srcs)
    stats = scene.overlap(0.02, 8.0)
    gains = lrp.camera_gains(stats, 3)
    want_stats = scene.want_overlap(0.02, 8.0)
    assert (stats.cpu().numpy() == want_stats).all()
    want_gains = lrp.camera_gains(want_stats, 3)
    assert gains.dtype == np.float32 and (gains.view(np.uint32) == want_gains.view(np.uint32)).all() and gains[0] > 1.0 > gains[2]
    scene.check(gains, 2, FEATHER, 1, "end to end")
