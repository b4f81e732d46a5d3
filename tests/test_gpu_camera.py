"""GPU: lrp_compose_cameras_device (include/lrp.h "compose, calibrated cameras"; csrc/lrp_camera_kernel.h) against the CPU model
of tests/camera_model.py — the definition per pixel, which tests/test_camera.py pins to float64 and to the existing lenses —
byte for byte, any NaN matching any NaN, both planes in every comparison.  The five target lenses x three samplers x three
modes at n 2 and 3 with a rig of mixed models, n 1 and 15, one and eight cameras, a fisheye that sees behind itself, the
identity (independent of the model), odd shapes, channel counts, post, no rotations, a side stream, planted special texels,
planes between guard bytes, and independence of kernel family and geometry cache."""
import numpy as np
import pytest

import camera_cases as cam
import camera_model as cmodel
import cases
import coverage_cases as cc

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True  # (the tests set the cache themselves)
FIRST, MEAN, FEATHER = 0, 1, 2
MODES = (FIRST, MEAN, FEATHER)
MODE_NAMES = {FIRST: "first", MEAN: "mean", FEATHER: "feather"}


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

    def __init__(self, lrp, torch, lout, size, cams, rots, channels=4, seed=700, planted=False):
        self.lrp, self.torch, self.lout, self.cams, self.rots, self.C = lrp, torch, lout, cams, rots, channels
        self.ow, self.oh = size
        self.host = [np.ascontiguousarray(s) for s in cam.sources(cams, channels, seed, planted)]
        self.dev = [torch.from_numpy(s).cuda() for s in self.host]
        self._want = {}

    @classmethod
    def rig(cls, lrp, torch, out_name="eqr_part", size=cam.OUT_SIZE, **kw):
        lout, cams, rots = cam.rig(lrp, out_name, size)
        return cls(lrp, torch, lout, size, cams, rots, **kw)

    def cameras(self):
        return [cam.product(self.lrp, c, d) for c, d in zip(self.cams, self.dev)]

    def out_image(self, data):
        return self.lrp.Image(self.lout, self.ow, self.oh, self.C, data)

    def expect(self, n, mode, interp, post=None):
        key = (n, mode, interp, post)
        if key not in self._want:
            self._want[key] = cmodel.compose(self.cams, self.host, self.lout, self.ow, self.oh, n, interp, self.rots, mode, post)
        return self._want[key]

    def compose(self, n, mode, interp, post=None, count=None, coverage=None, stream=None, fill=-1.0):
        d = self.torch.full((self.oh, self.ow, self.C), fill, dtype=self.torch.float32, device="cuda")
        planes = self.lrp.compose_cameras(self.cameras(), self.out_image(d), n, interp, self.rots, mode, post=post, count=count,
                                          coverage=coverage, stream=stream)
        return d, planes

    def check(self, n, mode, interp, what, post=None):
        d, (count, coverage) = self.compose(n, mode, interp, post=post, count=True, coverage=True)
        self.torch.cuda.synchronize()
        want, want_count, want_m = self.expect(n, mode, interp, post)
        what = f"{what}: n {n} {MODE_NAMES[mode]} interp {interp} post {post}"
        cases.assert_same_bits(d.cpu().numpy(), want, what)
        for plane in (count, coverage):
            assert plane.dtype == self.torch.uint8 and tuple(plane.shape) == (self.oh, self.ow)
        assert (count.cpu().numpy() == want_count).all(), f"{what}: count plane"
        assert (coverage.cpu().numpy() == want_m).all(), f"{what}: coverage plane"
        return want_count, want_m


@pytest.mark.parametrize("out_name", cam.OUT_LENSES)
def test_cells(lrp, torch_cuda, out_name):
    """Every instantiation: 5 target lenses x 3 samplers, every mode, n 2 and 3, the rig BROWN, FISHEYE, BROWN."""
    scene = Scene.rig(lrp, torch_cuda, out_name)
    for n in (2, 3):
        for interp in (0, 1, 2):
            for mode in MODES:
                count, m = scene.check(n, mode, interp, out_name)
        assert (m == 0).any() and ((m > 0) & (m < n * n)).any() and (m == n * n).any() and (count >= 2).any()
        # FIRST without a count plane leaves the source loop early: the same image, the same coverage
        d, (none, coverage) = scene.compose(n, FIRST, 2, coverage=True)
        torch_cuda.cuda.synchronize()
        assert none is None and (coverage.cpu().numpy() == m).all()
        cases.assert_same_bits(d.cpu().numpy(), scene.expect(n, FIRST, 2)[0], f"{out_name}: FIRST without a count plane")


@pytest.mark.parametrize("n", [1, 15])
def test_n(lrp, torch_cuda, n):
    scene = Scene.rig(lrp, torch_cuda, "eqr_part")
    for interp, mode in ((2, FEATHER), (0, FIRST), (1, MEAN)):
        count, m = scene.check(n, mode, interp, "n")
    assert (m == 0).any() and (m == n * n).any() and (count >= 2).any() and (n == 1 or ((m > 0) & (m < n * n)).any())


def test_one_camera_then_eight_nine_refused(lrp, torch_cuda):
    torch = torch_cuda
    pano = cc.lens(lrp, "eqr_full", 80, 48)
    for c, rot in ((cam.resolve(lrp, cam.RIG[0]), cam.RIG_ROTATIONS[0]), (cam.resolve(lrp, cam.RIG[1]), cam.RIG_ROTATIONS[1])):
        scene = Scene(lrp, torch, pano, (80, 48), [c], [cases.rotation(lrp, rot)])
        for mode in MODES:
            count, m = scene.check(2, mode, 2, "one camera")
        assert count.max() == 1 and (m == 0).any() and (m == 4).any()
    cams, rots = cam.eight(lrp)
    scene = Scene(lrp, torch, pano, (80, 48), cams, rots)
    for n in (2, 3):
        for mode in MODES:
            count, m = scene.check(n, mode, 2, "eight cameras")
    assert count.max() >= 3 and (m == 0).any() and {c["model"] for c in cams} == {cam.BROWN, cam.FISHEYE}
    with pytest.raises(lrp.LrpError) as e:  # nine: refused
        lrp.compose_cameras(scene.cameras() + scene.cameras()[:1], scene.out_image(torch.empty((48, 80, 4), device="cuda")), 2, 2)
    assert e.value.status == lrp.Status.BAD_ARG
    with pytest.raises(lrp.LrpError) as e:
        lrp.compose_cameras(scene.cameras(), scene.out_image(torch.empty((48, 80, 4), device="cuda")), 16, 2)
    assert e.value.status == lrp.Status.BAD_ARG


def test_fisheye_beyond_the_hemisphere(lrp, torch_cuda):
    """A 200 degree fisheye into a full panorama: some covered pixels have vz >= 0, which no source that folds through x / -z
    can deliver."""
    pano = cc.lens(lrp, "eqr_full", 96, 48)
    scene = Scene(lrp, torch_cuda, pano, (96, 48), [cam.FISHEYE_200], None)
    ray, _, _, covered = cmodel.detail(cam.FISHEYE_200, pano, 96, 48, 1)
    for interp in (0, 1, 2):
        _, m = scene.check(1, FIRST, interp, "200 degrees")
    assert (m == covered[:, :, 0]).all() and ((m == 1) & (ray[:, :, 0, 2] >= 0)).any() and (m == 0).any()
    scene.check(3, FEATHER, 2, "200 degrees")


def test_identity(lrp, torch_cuda):
    """Independent of the model: sx == x and sy == y exactly, so the launch returns the source bit for bit (bicubic too: the
    CPU test shows Catmull-Rom is exact at t = 0 for finite texels), coverage all 1, count all 1."""
    torch = torch_cuda
    src = cam.sources([cam.IDENTITY])[0]
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    for interp in (0, 1, 2):
        d = torch.full((32, 64, 4), -1.0, dtype=torch.float32, device="cuda")
        count, m = lrp.compose_cameras([cam.product(lrp, cam.IDENTITY, d_src)], lrp.Image(cam.identity_lens(lrp), 64, 32, 4, d), 1, interp,
                                       count=True, coverage=True)
        torch.cuda.synchronize()
        cases.assert_same_bits(d.cpu().numpy(), src, f"identity, interp {interp}")
        assert (count == 1).all() and (m == 1).all()


@pytest.mark.parametrize("size", [(1, 1), (33, 9), (31, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(lrp, torch_cuda, size):
    """One pixel; a row that ends one lane into the second tile and a ninth row; a tile that is one lane short."""
    for out_name in ("eqr_part", "rect18"):
        scene = Scene.rig(lrp, torch_cuda, out_name, size)
        for n in (2, 3):
            for mode in MODES:
                scene.check(n, mode, 2, f"{out_name} {size}")


@pytest.mark.parametrize("post", [None, (2.0, 3.0)], ids=["plain", "tonemap"])
@pytest.mark.parametrize("channels", [1, 3, 4, 5, 8, 9, 11])
def test_channels_and_post(lrp, torch_cuda, channels, post):
    """The run-time channel path, the tonemap on the first min(C, 3) channels of the covered pixels only, and — 9, 11 — a second
    launch for the channels beyond the eighth, which writes the planes again with the same bytes."""
    scene = Scene.rig(lrp, torch_cuda, "eqr_part", channels=channels, seed=800 + channels)
    for n, mode, interp in ((2, FIRST, 2), (3, MEAN, 1), (2, FEATHER, 0), (3, FEATHER, 2)):
        _, m = scene.check(n, mode, interp, f"C {channels}", post=post)
    d, _ = scene.compose(3, FEATHER, 2, post=post, fill=float("nan"))
    torch_cuda.cuda.synchronize()
    got = d.cpu().numpy()
    assert (m == 0).any() and ((got.view(np.uint32) == 0).all(axis=2) == (m == 0)).all(), "an uncovered pixel is +0.0 in every channel, and only it"


def test_no_rotations(lrp, torch_cuda):
    """rotations == NULL: no camera is rotated (and no multiplication happens)."""
    lout, cams, _ = cam.rig(lrp, "eqr_full")
    scene = Scene(lrp, torch_cuda, lout, cam.OUT_SIZE, cams, None)
    for mode in MODES:
        count, m = scene.check(2, mode, 2, "no rotations")
    assert count.max() == 3 and (m == 0).any() and ((m > 0) & (m < 4)).any()


def test_side_stream(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch)
    want, want_count, want_m = scene.expect(3, FEATHER, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d, (count, m) = scene.compose(3, FEATHER, 2, count=True, coverage=True, stream=side)
    side.synchronize()
    cases.assert_same_bits(d.cpu().numpy(), want, "side stream")
    assert (count.cpu().numpy() == want_count).all() and (m.cpu().numpy() == want_m).all()


def test_planted_special_texels(lrp, torch_cuda):
    """-0.0, denormals, inf, NaN and large values in the frames (any NaN matches any NaN)."""
    scene = Scene.rig(lrp, torch_cuda, planted=True)
    for n in (2, 3):
        for mode in MODES:
            scene.check(n, mode, 1, "planted")
    want = scene.expect(2, MEAN, 1)[0]
    assert any(np.signbit(s[s == 0]).any() for s in scene.host) and np.isnan(want).any() and np.isinf(want).any()


@pytest.mark.parametrize("which", ["count", "coverage", "both"])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_plane_alignment_and_guard_bytes(lrp, torch_cuda, offset, which):
    torch = torch_cuda
    for size in ((80, 48), (33, 9)):
        scene = Scene.rig(lrp, torch, "eqr_part", size)
        n_px = size[0] * size[1]
        bufs, views = {}, {}
        for name in ("count", "coverage"):
            if which in (name, "both"):
                buf = torch.full((64 + 4 + n_px + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
                first = (-buf.data_ptr()) % 4 + 64 + offset
                bufs[name], views[name] = (buf, first), buf[first:first + n_px]
                assert views[name].data_ptr() % 4 == offset
        for mode in (MEAN, FIRST):  # (FIRST without a count plane leaves the source loop early)
            d, got = scene.compose(3, mode, 1, count=views.get("count"), coverage=views.get("coverage"))
            torch.cuda.synchronize()
            want, want_count, want_m = scene.expect(3, mode, 1)
            assert want_count.max() >= 2 and ((want_m > 0) & (want_m < 9)).any()
            for i, (name, plane) in enumerate((("count", want_count), ("coverage", want_m))):
                if name not in views:
                    assert got[i] is None
                    continue
                assert got[i].data_ptr() == views[name].data_ptr()
                buf, first = bufs[name]
                host = buf.cpu().numpy()
                assert (host[first:first + n_px].reshape(size[1], size[0]) == plane).all(), f"{name} offset {offset} {size}"
                assert (host[:first] == 0xA5).all() and (host[first + n_px:] == 0xA5).all(), "guard bytes written"
            cases.assert_same_bits(d.cpu().numpy(), want, "the image beside misaligned planes")


def test_independent_of_kernel_family_and_geometry_cache(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch)
    want, want_count, want_m = scene.expect(2, FEATHER, 2)
    lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        d = torch.empty((scene.oh, scene.ow, 4), dtype=torch.float32, device="cuda")
        src = torch.from_numpy(cases.hash_noise(48, 64, 4, 1)).cuda()
        s0 = lrp.geometry_cache_stats()
        lrp.reproject(lrp.Image(cc.lens(lrp, "rect18", 64, 48), 64, 48, 4, src), scene.out_image(d), 1, 2, scene.rots[0])  # a geometry enters the cache
        torch.cuda.synchronize()
        s1 = lrp.geometry_cache_stats()
        assert s1["fills"] == s0["fills"] + 1, (s0, s1)
        for cache in (1, 0):
            lrp.debug_set("geo_cache", cache)
            for family in (0, 1, 2, 3):
                lrp.debug_kernel(family)
                got, (count, m) = scene.compose(2, FEATHER, 2, count=True, coverage=True)
                torch.cuda.synchronize()
                cases.assert_same_bits(got.cpu().numpy(), want, f"kernel family {family}, cache {cache}")
                assert (count.cpu().numpy() == want_count).all() and (m.cpu().numpy() == want_m).all()
        assert lrp.geometry_cache_stats() == s1, "a compose_cameras call moved the cache counters"
    finally:
        lrp.release_cached_tables()
