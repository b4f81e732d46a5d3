"""GPU: lrp_compose_ss_device (include/lrp.h "compose, supersampled"; csrc/lrp_compose_ss_kernel.h) against the CPU model of
tests/compose_ss_model.py — the definition per pixel on the coverage model's lenses, samplers and coverage test, which
tests/test_compose_ss.py pins to the definition and tests/test_gpu_coverage.py to the kernels' coordinates — byte for byte, any
NaN matching any NaN.  All 30 cells x three samplers x three modes at n 2 and 3, the discriminating cases of
tests/compose_ss_cases.py at n 2, 3, 4, 5 and 15, n = 1 against compose() and one source against reproject(num_samples=n) on
the device, one and eight sources, both planes between guard bytes, odd shapes, channel counts, post, no rotations, a side
stream, planted special texels, independence of kernel family and geometry cache, and the cube's seam counts."""
import numpy as np
import pytest

import cases
import compose_cases as cs
import compose_ss_cases as ss
import compose_ss_model as ssm
import coverage_cases as cc

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
    """A case on the device and on the host: the sources, their rotations, the launch and the model's expectation."""

    def __init__(self, lrp, torch, case, channels=4, seed=400, planted=False, no_rotations=False):
        self.lrp, self.torch, self.case, self.C = lrp, torch, case, channels
        self.ow, self.oh = case["out_size"]
        self.lout, self.lins = cs.lenses(lrp, case)
        self.sizes = [size for _, size, _ in case["sources"]]
        self.rots = None if no_rotations else ss.rotations(lrp, case)
        self.host = [np.ascontiguousarray(s) for s in ss.sources(case, channels, seed, planted)]
        self.srcs = [torch.from_numpy(s).cuda() for s in self.host]
        self._want = {}

    def images(self):
        return [self.lrp.Image(lin, w, h, self.C, d) for lin, (w, h), d in zip(self.lins, self.sizes, self.srcs)]

    def out_image(self, data):
        return self.lrp.Image(self.lout, self.ow, self.oh, self.C, data)

    def expect(self, n, mode, interp, post=None):
        key = (n, mode, interp, post)
        if key not in self._want:
            self._want[key] = ssm.compose(self.lins, self.host, self.lout, self.ow, self.oh, n, interp, self.rots, mode, post)
        return self._want[key]

    def compose(self, n, mode, interp, post=None, count=None, coverage=None, stream=None, fill=-1.0):
        d = self.torch.full((self.oh, self.ow, self.C), fill, dtype=self.torch.float32, device="cuda")
        planes = self.lrp.compose_ss(self.images(), self.out_image(d), n, interp, self.rots, mode, post=post, count=count, coverage=coverage,
                                     stream=stream)
        return d, planes

    def check(self, n, mode, interp, what, post=None):
        d, (count, coverage) = self.compose(n, mode, interp, post=post, count=True, coverage=True)
        self.torch.cuda.synchronize()
        want, want_count, want_m = self.expect(n, mode, interp, post)
        what = f"{what}: n {n} {cs.MODE_NAMES[mode]} interp {interp} post {post}"
        cases.assert_same_bits(d.cpu().numpy(), want, what)
        for plane in (count, coverage):
            assert plane.dtype == self.torch.uint8 and tuple(plane.shape) == (self.oh, self.ow)
        assert (count.cpu().numpy() == want_count).all(), f"{what}: count plane"
        assert (coverage.cpu().numpy() == want_m).all(), f"{what}: coverage plane"
        return want_count, want_m


CELLS = cc.cells()


@pytest.mark.parametrize("cell", CELLS, ids=[f"{o}<-{s}" for o, s, _ in CELLS])
def test_cells(lrp, torch_cuda, cell):
    scene = Scene(lrp, torch_cuda, cs.cell_case(*cell))
    for n in ss.CELL_N:
        for interp in (0, 1, 2):
            for mode in cs.MODES:
                count, m = scene.check(n, mode, interp, str(cell))
        assert (count >= 2).any() and (m > 0).any(), "a cell without overlap"  # (the covering sets differ: tests/test_compose_ss.py)


CASE_RUNS = ss.DISCRIMINATING + [(case, n) for case in dict((id(c), c) for c, _ in ss.DISCRIMINATING).values() for n in ss.LARGE_N]


@pytest.mark.parametrize("item", CASE_RUNS, ids=ss.case_id)
def test_cases(lrp, torch_cuda, item):
    case, n = item
    scene = Scene(lrp, torch_cuda, case)
    for interp in (2, 0):
        for mode in cs.MODES:
            count, m = scene.check(n, mode, interp, case["name"])
    assert ((m > 0) & (m < n * n)).mean() >= ss.PARTIAL_MIN and (m == 0).any() and (m == n * n).any() and (count >= 2).any()


@pytest.mark.parametrize("planted", [False, True], ids=["noise", "planted"])
def test_n1_is_compose_on_the_device(lrp, torch_cuda, planted):
    """n == 1: the bytes of lrp_compose_device, except that a -0.0f channel becomes +0.0f (with planted texels alone); count is
    equal; coverage is k > 0."""
    torch = torch_cuda
    for case in (cs.OVERLAP_CASES[0], cs.OVERLAP_CASES[2]):
        scene = Scene(lrp, torch, case, planted=planted)
        for interp in (0, 1, 2):
            for mode in cs.MODES:
                ref = torch.full((scene.oh, scene.ow, 4), -1.0, dtype=torch.float32, device="cuda")
                k = lrp.compose(scene.images(), scene.out_image(ref), interp, scene.rots, mode, count=True)
                d, (count, coverage) = scene.compose(1, mode, interp, count=True, coverage=True)
                torch.cuda.synchronize()
                want = ref.cpu().numpy()
                if planted:
                    want = np.where(want == 0, np.float32(0.0), want)  # -0.0f -> +0.0f
                else:
                    assert not (np.signbit(want) & (want == 0)).any()
                cases.assert_same_bits(d.cpu().numpy(), want, f"{case['name']} {cs.MODE_NAMES[mode]} interp {interp}")
                assert torch.equal(count, k) and torch.equal(coverage, (k > 0).to(torch.uint8)) and (k >= 2).any() and (k == 0).any()


@pytest.mark.parametrize("n", [2, 3, 4])
def test_one_source_is_reproject_where_fully_covered(lrp, torch_cuda, n):
    """One source, FIRST or MEAN, a pixel with m == n * n: bit for bit what reproject(num_samples=n) stores; and against the model."""
    torch = torch_cuda
    case = cs._case("one", "eqr_full", (80, 48), [("rect18", (64, 48), cc.GENERAL)])
    scene = Scene(lrp, torch, case)
    for interp in (0, 1, 2):
        ref = torch.full((48, 80, 4), -1.0, dtype=torch.float32, device="cuda")
        lrp.reproject(scene.images()[0], scene.out_image(ref), n, interp, scene.rots[0])
        plane = lrp.coverage(scene.images()[0], scene.out_image(None), n, scene.rots[0], device=0)
        for mode in (cs.FIRST, cs.MEAN):
            d, (count, m) = scene.compose(n, mode, interp, count=True, coverage=True)
            torch.cuda.synchronize()
            assert torch.equal(m, plane) and torch.equal(count, (plane > 0).to(torch.uint8))
            full = (m == n * n).cpu().numpy()
            assert 0.05 < full.mean() < 0.95
            cases.assert_same_bits(d.cpu().numpy()[full], ref.cpu().numpy()[full], f"n {n} interp {interp} {cs.MODE_NAMES[mode]}")
            scene.check(n, mode, interp, "one source")


def test_eight_sources(lrp, torch_cuda):
    sources = [("rect18", (64 - 8 * (i % 2), 48), (35.0 * i, 10.0 * (i % 3) - 10.0, 0.0)) for i in range(8)]
    scene = Scene(lrp, torch_cuda, cs._case("rig8", "eqr_full", (80, 48), sources))
    for n in (2, 3):
        for mode in cs.MODES:
            count, m = scene.check(n, mode, 2, "eight sources")
    assert count.max() >= 3 and (m == 0).any()
    with pytest.raises(lrp.LrpError) as e:  # nine: refused
        lrp.compose_ss(scene.images() + scene.images()[:1], scene.out_image(torch_cuda.empty((48, 80, 4), device="cuda")), 2, 2)
    assert e.value.status == lrp.Status.BAD_ARG
    with pytest.raises(lrp.LrpError) as e:
        lrp.compose_ss(scene.images(), scene.out_image(torch_cuda.empty((48, 80, 4), device="cuda")), 16, 2)
    assert e.value.status == lrp.Status.BAD_ARG


@pytest.mark.parametrize("which", ["count", "coverage", "both"])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_plane_alignment_and_guard_bytes(lrp, torch_cuda, offset, which):
    torch = torch_cuda
    for size in ((80, 48), (33, 9)):
        scene = Scene(lrp, torch, dict(cs.OVERLAP_CASES[0], out_size=size))
        n_px = size[0] * size[1]
        bufs, views = {}, {}
        for name in ("count", "coverage"):
            if which in (name, "both"):
                buf = torch.full((64 + 4 + n_px + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
                first = (-buf.data_ptr()) % 4 + 64 + offset
                bufs[name], views[name] = (buf, first), buf[first:first + n_px]
                assert views[name].data_ptr() % 4 == offset
        for mode in (cs.MEAN, cs.FIRST):  # (FIRST without a count plane leaves the source loop early)
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


@pytest.mark.parametrize("size", [(1, 1), (33, 9), (31, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(lrp, torch_cuda, size):
    """One pixel; a row that ends one lane into the second tile and a ninth row; a tile that is one lane short."""
    for case in (cs.OVERLAP_CASES[0], cs.OVERLAP_CASES[2]):
        scene = Scene(lrp, torch_cuda, dict(case, out_size=size))
        for n in (2, 3):
            for mode in cs.MODES:
                scene.check(n, mode, 2, f"{case['name']} {size}")


@pytest.mark.parametrize("post", [None, (2.0, 3.0)], ids=["plain", "tonemap"])
@pytest.mark.parametrize("channels", [1, 3, 4, 5, 8, 9, 11])
def test_channels_and_post(lrp, torch_cuda, channels, post):
    """The run-time channel path, the tonemap on the first min(C, 3) channels of the covered pixels only, and — 9, 11 — a second
    launch for the channels beyond the eighth, which writes the planes again with the same bytes."""
    scene = Scene(lrp, torch_cuda, cs.OVERLAP_CASES[0], channels=channels, seed=500 + channels)
    for n, mode, interp in ((2, cs.FIRST, 2), (3, cs.MEAN, 1), (2, cs.FEATHER, 0), (3, cs.FEATHER, 2)):
        _, m = scene.check(n, mode, interp, f"C {channels}", post=post)
    d, _ = scene.compose(3, cs.FEATHER, 2, post=post, fill=float("nan"))
    torch_cuda.cuda.synchronize()
    got = d.cpu().numpy()
    assert ((got.view(np.uint32) == 0).all(axis=2) == (m == 0)).all(), "an uncovered pixel is +0.0 in every channel, and only it"


def test_no_rotations(lrp, torch_cuda):
    """rotations == NULL: no source is rotated (and no multiplication happens)."""
    case = cs._case("unrotated", "eqr_full", (80, 48), [("rect18", (64, 48), None), ("rect12", (48, 32), None), ("rect35", (64, 48), None)])
    scene = Scene(lrp, torch_cuda, case, no_rotations=True)
    for mode in cs.MODES:
        count, m = scene.check(2, mode, 2, "no rotations")
    assert count.max() == 3 and (m == 0).any() and ((m > 0) & (m < 4)).any()


def test_side_stream(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene(lrp, torch, cs.OVERLAP_CASES[2])
    want, want_count, want_m = scene.expect(3, cs.FEATHER, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d, (count, m) = scene.compose(3, cs.FEATHER, 2, count=True, coverage=True, stream=side)
    side.synchronize()
    cases.assert_same_bits(d.cpu().numpy(), want, "side stream")
    assert (count.cpu().numpy() == want_count).all() and (m.cpu().numpy() == want_m).all()


def test_planted_special_texels(lrp, torch_cuda):
    """-0.0, denormals, inf, NaN and large values in the sources (any NaN matches any NaN)."""
    scene = Scene(lrp, torch_cuda, cs.OVERLAP_CASES[0], planted=True)
    for n in (2, 3):
        for mode in cs.MODES:
            scene.check(n, mode, 1, "planted")
    assert any(np.signbit(s[s == 0]).any() for s in scene.host) and not np.isfinite(scene.expect(2, cs.MEAN, 1)[0]).all()


def test_independent_of_kernel_family_and_geometry_cache(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene(lrp, torch, cs.OVERLAP_CASES[2])
    want, want_count, want_m = scene.expect(2, cs.FEATHER, 2)
    lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        d = torch.empty((scene.oh, scene.ow, 4), dtype=torch.float32, device="cuda")
        s0 = lrp.geometry_cache_stats()
        lrp.reproject(scene.images()[0], scene.out_image(d), 1, 2, scene.rots[0])  # the geometry of source 0 enters the cache
        torch.cuda.synchronize()
        s1 = lrp.geometry_cache_stats()
        assert s1["fills"] == s0["fills"] + 1, (s0, s1)
        for cache in (1, 0):
            lrp.debug_set("geo_cache", cache)
            for family in (0, 1, 2, 3):
                lrp.debug_kernel(family)
                got, (count, m) = scene.compose(2, cs.FEATHER, 2, count=True, coverage=True)
                torch.cuda.synchronize()
                cases.assert_same_bits(got.cpu().numpy(), want, f"kernel family {family}, cache {cache}")
                assert (count.cpu().numpy() == want_count).all() and (m.cpu().numpy() == want_m).all()
        assert lrp.geometry_cache_stats() == s1, "a compose_ss call moved the cache counters"
    finally:
        lrp.release_cached_tables()


def test_cube_seam_counts(lrp, torch_cuda):
    """The 14 uncovered seam pixels of n = 1 (tests/compose_cases.py CUBE_SEAMS) and the model's counts at n = 2."""
    scene = Scene(lrp, torch_cuda, cs.CUBE)
    _, m1 = scene.check(1, cs.FIRST, 2, "cube")
    assert int((m1 == 0).sum()) == cs.CUBE_SEAMS["k0"]
    for mode in cs.MODES:
        count, m = scene.check(2, mode, 2, "cube")
    want = ss.CUBE_SEAMS_N2
    assert int((m == 0).sum()) == want["m0"] and int(((m > 0) & (m < 4)).sum()) == want["partial"] and int((count >= 2).sum()) == want["count2"]
