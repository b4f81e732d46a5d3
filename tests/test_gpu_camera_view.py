"""GPU: lrp_camera_view_device (include/lrp.h "calibrated camera as the target"; csrc/lrp_camview_kernel.h) against the CPU
model of tests/camera_view_model.py — the definition per pixel, which tests/test_camera_view.py pins to float64, to the
rectilinear lens and to lrp_camera_unproject — byte for byte, any NaN matching any NaN, both planes in every comparison.  The
six target cameras x three samplers x three modes at n 2 and 3 with a rig of mixed models, n 1 and 15 on the clipped target,
the identity (independent of the model), odd shapes, channel counts, post, eight cameras, camera to camera in both directions,
no rotations, a side stream, planted special texels, planes between guard bytes, and the geometry cache untouched."""
import numpy as np
import pytest

import camera_cases as cam
import camera_view_cases as cvc
import camera_view_model as cvmodel
import cases

pytestmark = pytest.mark.gpu
FIRST, MEAN, FEATHER = 0, 1, 2
MODES = (FIRST, MEAN, FEATHER)
MODE_NAMES = {FIRST: "first", MEAN: "mean", FEATHER: "feather"}


class Scene:
    """Cameras on the device and on the host and a target camera: the frames, the rotations, the launch and the model's expectation."""

    def __init__(self, lrp, torch, target, cams, rots, channels=4, seed=900, planted=False):
        self.lrp, self.torch, self.target, self.cams, self.rots, self.C = lrp, torch, target, cams, rots, channels
        self.ow, self.oh = target["size"]
        self.host = [np.ascontiguousarray(s) for s in cam.sources(cams, channels, seed, planted)]
        self.dev = [torch.from_numpy(s).cuda() for s in self.host]
        self._want = {}

    @classmethod
    def rig(cls, lrp, torch, name="brown_clipped", size=None, **kw):
        cams, rots = cvc.rig(lrp)
        return cls(lrp, torch, cvc.target(lrp, name) if size is None else cvc.small_target(lrp, name, size), cams, rots, **kw)

    def cameras(self):
        return [cam.product(self.lrp, c, d) for c, d in zip(self.cams, self.dev)]

    def expect(self, n, mode, interp, post=None):
        key = (n, mode, interp, post)
        if key not in self._want:
            self._want[key] = cvmodel.compose(self.cams, self.host, self.target, n, interp, self.rots, mode, post)
        return self._want[key]

    def view(self, n, mode, interp, post=None, count=None, coverage=None, stream=None, fill=-1.0):
        d = self.torch.full((self.oh, self.ow, self.C), fill, dtype=self.torch.float32, device="cuda")
        planes = self.lrp.camera_view(self.cameras(), cam.product(self.lrp, self.target), d, n, interp, self.rots, mode, post=post, count=count,
                                      coverage=coverage, stream=stream)
        return d, planes

    def check(self, n, mode, interp, what, post=None):
        d, (count, coverage) = self.view(n, mode, interp, post=post, count=True, coverage=True)
        self.torch.cuda.synchronize()
        want, want_count, want_m = self.expect(n, mode, interp, post)
        what = f"{what}: n {n} {MODE_NAMES[mode]} interp {interp} post {post}"
        cases.assert_same_bits(d.cpu().numpy(), want, what)
        for plane in (count, coverage):
            assert plane.dtype == self.torch.uint8 and tuple(plane.shape) == (self.oh, self.ow)
        assert (count.cpu().numpy() == want_count).all(), f"{what}: count plane"
        assert (coverage.cpu().numpy() == want_m).all(), f"{what}: coverage plane"
        return want_count, want_m


@pytest.mark.parametrize("name", list(cvc.TARGETS))
def test_cells(lrp, torch_cuda, name):
    """Every instantiation: 2 target models x 3 samplers, every mode, n 2 and 3, six target cameras, the rig BROWN, FISHEYE, BROWN."""
    scene = Scene.rig(lrp, torch_cuda, name)
    for n in (2, 3):
        for interp in (0, 1, 2):
            for mode in MODES:
                count, m = scene.check(n, mode, interp, name)
        assert cam.discriminates(count, m, n)
        # FIRST without a count plane leaves the source loop early: the same image, the same coverage
        d, (none, coverage) = scene.view(n, FIRST, 2, coverage=True)
        torch_cuda.cuda.synchronize()
        assert none is None and (coverage.cpu().numpy() == m).all()
        cases.assert_same_bits(d.cpu().numpy(), scene.expect(n, FIRST, 2)[0], f"{name}: FIRST without a count plane")


@pytest.mark.parametrize("n", [1, 15])
def test_n(lrp, torch_cuda, n):
    scene = Scene.rig(lrp, torch_cuda, "brown_clipped")
    for interp, mode in ((2, FEATHER), (0, FIRST), (1, MEAN)):
        count, m = scene.check(n, mode, interp, "n")
    assert (m == 0).any() and (m == n * n).any() and (count >= 2).any() and (n == 1 or ((m > 0) & (m < n * n)).any())


def test_identity(lrp, torch_cuda):
    """Independent of the model: the target is the camera of the only source, no rotation, n = 1, NEAREST.  The round trip
    through the inverse and the forward polynomial is 1e-5 px and NEAREST needs less than 0.5: out == source bit for bit,
    coverage all ones."""
    torch = torch_cuda
    c = cam.resolve(lrp, cam.camera(cam.BROWN, (64, 48), 58.0, 59.0, 32.4, 22.9, cam.BROWN_MILD))
    src = cam.sources([c])[0]
    d_src = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d = torch.full((48, 64, 4), -1.0, dtype=torch.float32, device="cuda")
    count, m = lrp.camera_view([cam.product(lrp, c, d_src)], cam.product(lrp, c), d, 1, 0, count=True, coverage=True)
    torch.cuda.synchronize()
    cases.assert_same_bits(d.cpu().numpy(), src, "identity")
    assert (count == 1).all() and (m == 1).all()


@pytest.mark.parametrize("size", [(1, 1), (33, 9), (31, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(lrp, torch_cuda, size):
    """One pixel; a row that ends one lane into the second tile and a ninth row; a tile that is one lane short."""
    for name in ("brown_clipped", "fisheye"):
        scene = Scene.rig(lrp, torch_cuda, name, size)
        for n in (2, 3):
            for mode in MODES:
                scene.check(n, mode, 2, f"{name} {size}")


@pytest.mark.parametrize("post", [None, (2.0, 3.0)], ids=["plain", "tonemap"])
@pytest.mark.parametrize("channels", [1, 3, 4, 5, 8, 9, 11])
def test_channels_and_post(lrp, torch_cuda, channels, post):
    """The run-time channel path, the tonemap on the first min(C, 3) channels of the covered pixels only, and — 9, 11 — a second
    launch for the channels beyond the eighth, which writes the planes again with the same bytes."""
    scene = Scene.rig(lrp, torch_cuda, "brown_clipped", channels=channels, seed=1000 + channels)
    for n, mode, interp in ((2, FIRST, 2), (3, MEAN, 1), (2, FEATHER, 0), (3, FEATHER, 2)):
        _, m = scene.check(n, mode, interp, f"C {channels}", post=post)
    d, _ = scene.view(3, FEATHER, 2, post=post, fill=float("nan"))
    torch_cuda.cuda.synchronize()
    got = d.cpu().numpy()
    assert (m == 0).any() and ((got.view(np.uint32) == 0).all(axis=2) == (m == 0)).all(), "an uncovered pixel is +0.0 in every channel, and only it"


def test_eight_cameras_nine_refused(lrp, torch_cuda):
    torch = torch_cuda
    cams, rots = cam.eight(lrp)
    scene = Scene(lrp, torch, cvc.target(lrp, "fisheye_clipped"), cams, rots)
    for n in (2, 3):
        for mode in MODES:
            count, m = scene.check(n, mode, 2, "eight cameras")
    assert count.max() >= 3 and (m == 0).any() and {c["model"] for c in cams} == {cam.BROWN, cam.FISHEYE}
    out = torch.empty((scene.oh, scene.ow, 4), device="cuda")
    with pytest.raises(lrp.LrpError) as e:  # nine: refused
        lrp.camera_view(scene.cameras() + scene.cameras()[:1], cam.product(lrp, scene.target), out, 2, 2)
    assert e.value.status == lrp.Status.BAD_ARG
    with pytest.raises(lrp.LrpError) as e:
        lrp.camera_view(scene.cameras(), cam.product(lrp, scene.target), out, 16, 2)
    assert e.value.status == lrp.Status.BAD_ARG


def test_camera_to_camera(lrp, torch_cuda):
    """A Kannala-Brandt target from one Brown-Conrady source, and the reverse: the frame of camera A as camera B would have seen it."""
    for src, name in ((cam.RIG[0], "fisheye"), (cam.RIG[1], "brown_mild")):
        target = cvc.target(lrp, name)
        assert src["model"] != target["model"]
        scene = Scene(lrp, torch_cuda, target, [cam.resolve(lrp, src)], [cases.rotation(lrp, (5.0, -3.0, 2.0))])
        for mode in MODES:
            count, m = scene.check(2, mode, 2, f"model {src['model']} -> {name}")
        assert count.max() == 1 and (m == 0).any() and (m == 4).any()


def test_no_rotations(lrp, torch_cuda):
    """rotations == NULL: no camera is rotated (and no multiplication happens)."""
    cams, _ = cvc.rig(lrp)
    scene = Scene(lrp, torch_cuda, cvc.target(lrp, "fisheye"), cams, None)
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
        d, (count, m) = scene.view(3, FEATHER, 2, count=True, coverage=True, stream=side)
    side.synchronize()
    cases.assert_same_bits(d.cpu().numpy(), want, "side stream")
    assert (count.cpu().numpy() == want_count).all() and (m.cpu().numpy() == want_m).all()


def test_planted_special_texels(lrp, torch_cuda):
    """-0.0, denormals, inf, NaN and large values in the frames (any NaN matches any NaN)."""
    scene = Scene.rig(lrp, torch_cuda, "brown_wide", planted=True)
    for n in (2, 3):
        for mode in MODES:
            scene.check(n, mode, 1, "planted")
    want = scene.expect(2, MEAN, 1)[0]
    assert any(np.signbit(s[s == 0]).any() for s in scene.host) and np.isnan(want).any() and np.isinf(want).any()


@pytest.mark.parametrize("which", ["count", "coverage", "both"])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_plane_alignment_and_guard_bytes(lrp, torch_cuda, offset, which):
    torch = torch_cuda
    for size in ((48, 36), (33, 9)):
        scene = Scene.rig(lrp, torch, "brown_clipped", size)
        n_px = size[0] * size[1]
        bufs, views = {}, {}
        for name in ("count", "coverage"):
            if which in (name, "both"):
                buf = torch.full((64 + 4 + n_px + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
                first = (-buf.data_ptr()) % 4 + 64 + offset
                bufs[name], views[name] = (buf, first), buf[first:first + n_px]
                assert views[name].data_ptr() % 4 == offset
        for mode in (MEAN, FIRST):  # (FIRST without a count plane leaves the source loop early)
            d, got = scene.view(3, mode, 1, count=views.get("count"), coverage=views.get("coverage"))
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


def test_geometry_cache_counters_do_not_move(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene.rig(lrp, torch)
    want, want_count, want_m = scene.expect(2, FEATHER, 2)
    prev_cache = lrp.debug_set("geo_cache", 1)
    try:
        s0 = lrp.geometry_cache_stats()
        got, (count, m) = scene.view(2, FEATHER, 2, count=True, coverage=True)
        torch.cuda.synchronize()
        cases.assert_same_bits(got.cpu().numpy(), want, "with the geometry cache on")
        assert (count.cpu().numpy() == want_count).all() and (m.cpu().numpy() == want_m).all()
        assert lrp.geometry_cache_stats() == s0, "a camera_view call moved the cache counters"
    finally:
        lrp.debug_set("geo_cache", prev_cache)
