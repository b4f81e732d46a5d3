"""GPU: lrp_compose_device (include/lrp.h "compose"; csrc/lrp_compose_kernel.h) against the composition, by the definition, of what
the EXISTING public calls deliver — per source one reproject() and one coverage(), downloaded and composed in numpy float32
(tests/compose_cases.py expect(): a select, or adds and one division; the FEATHER weights from the coordinates of the CPU model,
which tests/test_coverage.py proves equal to the kernels') — byte for byte.  All 30 cells x three samplers x three modes, the
discriminating cases of tests/compose_cases.py, the cube and its seam counts, one and eight sources, the count plane between guard
bytes, odd shapes, channel counts, post, no rotations, a side stream, independence of kernel family and geometry cache, and
one mid-size frame by checksum."""
import numpy as np
import pytest

import cases
import compose_cases as cs
import coverage_cases as cc
import coverage_model as model

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
    """A case on the device: the sources, their rotations and — made once per sampler, by the existing calls — what every
    source renders and covers alone."""

    def __init__(self, lrp, torch, case, channels=4, seed=200, planted=False, no_rotations=False):
        self.lrp, self.torch, self.case, self.C = lrp, torch, case, channels
        self.ow, self.oh = case["out_size"]
        self.lout, self.lins = cs.lenses(lrp, case)
        self.sizes = [size for _, size, _ in case["sources"]]
        self.rots = None if no_rotations else [cases.rotation(lrp, deg) for _, _, deg in case["sources"]]
        self.srcs = []
        for i, (w, h) in enumerate(self.sizes):  # (no zero texel without planted ones: a zero pixel is an uncovered one)
            src = cases.hash_noise(h, w, channels, seed + i, planted=planted) + (np.float32(0.0) if planted else np.float32(0.25))
            self.srcs.append(torch.from_numpy(np.ascontiguousarray(src)).cuda())
        self._parts, self._weights = {}, None

    def rot(self, i):
        return None if self.rots is None else self.rots[i]

    def images(self):
        return [self.lrp.Image(lin, w, h, self.C, d) for lin, (w, h), d in zip(self.lins, self.sizes, self.srcs)]

    def out_image(self, data):
        return self.lrp.Image(self.lout, self.ow, self.oh, self.C, data)

    def parts(self, interp):
        if interp not in self._parts:
            lrp, torch = self.lrp, self.torch
            renders, planes = [], []
            for i, im in enumerate(self.images()):
                d = torch.full((self.oh, self.ow, self.C), -1.0, dtype=torch.float32, device="cuda")
                lrp.reproject(im, self.out_image(d), 1, interp, self.rot(i))
                p = lrp.coverage(im, self.out_image(None), 1, self.rot(i), device=0)
                torch.cuda.synchronize()
                renders.append(d.cpu().numpy())
                planes.append(p.cpu().numpy())
            self._parts[interp] = (renders, planes)
        return self._parts[interp]

    def weights(self):
        if self._weights is None:
            self._weights = []
            for i, (lin, (w, h)) in enumerate(zip(self.lins, self.sizes)):
                _, sxy, _ = model.coverage(lin, w, h, self.lout, self.ow, self.oh, 1, self.rot(i), detail=True)
                self._weights.append(cs.feather_weight(sxy[:, :, 0, :], w, h, cs.wraps(self.case["sources"][i][0])))
        return self._weights

    def expect(self, mode, interp, post=None):
        renders, planes = self.parts(interp)
        want, k = cs.expect(mode, renders, planes, self.weights() if mode == cs.FEATHER else None)
        if post is not None:  # the existing stand-alone post_process on the composed image; the uncovered pixels keep +0.0
            d = self.torch.from_numpy(want).cuda()
            self.lrp.post_process(self.out_image(d), post[0], post[1])
            self.torch.cuda.synchronize()
            want = d.cpu().numpy()
            want[k == 0] = np.float32(0.0)
        return want, k

    def compose(self, mode, interp, post=None, count=None, stream=None, fill=-1.0):
        d = self.torch.full((self.oh, self.ow, self.C), fill, dtype=self.torch.float32, device="cuda")
        plane = self.lrp.compose(self.images(), self.out_image(d), interp, self.rots, mode, post=post, count=count, stream=stream)
        return d, plane

    def check(self, mode, interp, what, post=None):
        d, plane = self.compose(mode, interp, post=post, count=True)
        self.torch.cuda.synchronize()
        want, k = self.expect(mode, interp, post)
        cases.assert_same_bits(d.cpu().numpy(), want, f"{what}: {cs.MODE_NAMES[mode]} interp {interp} post {post}")
        assert plane.dtype == self.torch.uint8 and tuple(plane.shape) == (self.oh, self.ow)
        assert (plane.cpu().numpy() == k).all(), f"{what}: count plane"
        return k


CELLS = cc.cells()


@pytest.mark.parametrize("cell", CELLS, ids=[f"{o}<-{s}" for o, s, _ in CELLS])
def test_cells(lrp, torch_cuda, cell):
    scene = Scene(lrp, torch_cuda, cs.cell_case(*cell))
    for interp in (0, 1, 2):
        for mode in cs.MODES:
            k = scene.check(mode, interp, str(cell))
    assert (k >= 2).any() and (k == 1).any(), "a cell without overlap checks no accumulation"


@pytest.mark.parametrize("case", cs.CASES, ids=[c["name"] for c in cs.CASES])
def test_cases(lrp, torch_cuda, case):
    scene = Scene(lrp, torch_cuda, case)
    for interp in (2, 0):
        for mode in cs.MODES:
            k = scene.check(mode, interp, case["name"])
    if case is cs.CUBE:  # the seams: the model's figures (tests/test_compose.py), recorded in DESIGN.md section 12
        assert int((k == 0).sum()) == cs.CUBE_SEAMS["k0"] and int((k >= 2).sum()) == cs.CUBE_SEAMS["k2"]
    else:
        assert min((k == 0).mean(), (k == 1).mean(), (k >= 2).mean()) >= 0.05


def test_planted_special_texels(lrp, torch_cuda):
    """-0.0, denormals, inf, NaN and large values in the sources (any NaN matches any NaN)."""
    scene = Scene(lrp, torch_cuda, cs.OVERLAP_CASES[0], planted=True)
    for mode in cs.MODES:
        scene.check(mode, 1, "planted")


def test_single_source_first_is_reproject_then_mask(lrp, torch_cuda):
    torch = torch_cuda
    case = cs._case("one", "eqr_full", (96, 48), [("rect18", (64, 48), cc.GENERAL)])
    scene = Scene(lrp, torch, case)
    for interp in (0, 1, 2):
        im = scene.images()[0]
        d_ref = torch.full((48, 96, 4), -1.0, dtype=torch.float32, device="cuda")
        lrp.reproject(im, scene.out_image(d_ref), 1, interp, scene.rot(0))
        plane = lrp.coverage(im, scene.out_image(d_ref), 1, scene.rot(0), mask_image=True)
        d, count = scene.compose(cs.FIRST, interp, count=True)
        torch.cuda.synchronize()
        assert torch.equal(d.view(torch.int32), d_ref.view(torch.int32)), f"interp {interp}"
        assert torch.equal(count, plane) and 0.05 < float((plane == 0).float().mean()) < 0.95


def test_eight_sources(lrp, torch_cuda):
    sources = [("rect18", (64 - 8 * (i % 2), 48), (35.0 * i, 10.0 * (i % 3) - 10.0, 0.0)) for i in range(8)]
    scene = Scene(lrp, torch_cuda, cs._case("rig8", "eqr_full", (80, 48), sources))
    for mode in cs.MODES:
        k = scene.check(mode, 2, "eight sources")
    assert k.max() >= 3 and (k == 0).any()
    with pytest.raises(lrp.LrpError) as e:  # nine: refused
        lrp.compose(scene.images() + scene.images()[:1], scene.out_image(torch_cuda.empty((48, 80, 4), device="cuda")), 2)
    assert e.value.status == lrp.Status.BAD_ARG


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_count_plane_alignment_and_guard_bytes(lrp, torch_cuda, offset):
    torch = torch_cuda
    for size in ((80, 48), (33, 9)):
        scene = Scene(lrp, torch, dict(cs.OVERLAP_CASES[0], out_size=size))
        n_px = size[0] * size[1]
        buf = torch.full((64 + 4 + n_px + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        first = (-buf.data_ptr()) % 4 + 64 + offset
        view = buf[first:first + n_px]
        assert view.data_ptr() % 4 == offset
        d, got = scene.compose(cs.MEAN, 1, count=view)
        torch.cuda.synchronize()
        assert got.data_ptr() == view.data_ptr()
        want, k = scene.expect(cs.MEAN, 1)
        planes = scene.parts(1)[1]
        assert (k == np.sum([p > 0 for p in planes], axis=0)).all() and k.max() >= 2
        host = buf.cpu().numpy()
        assert (host[first:first + n_px].reshape(size[1], size[0]) == k).all(), f"offset {offset} {size}"
        assert (host[:first] == 0xA5).all() and (host[first + n_px:] == 0xA5).all(), "guard bytes written"
        cases.assert_same_bits(d.cpu().numpy(), want, "the image beside a misaligned plane")


@pytest.mark.parametrize("size", [(1, 1), (33, 9), (31, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(lrp, torch_cuda, size):
    """One pixel; a row that ends one lane into the second tile and a ninth row; a tile that is one lane short."""
    for case in (cs.OVERLAP_CASES[0], cs.OVERLAP_CASES[2]):
        scene = Scene(lrp, torch_cuda, dict(case, out_size=size))
        for mode in cs.MODES:
            scene.check(mode, 2, f"{case['name']} {size}")


@pytest.mark.parametrize("post", [None, (2.0, 3.0)], ids=["plain", "tonemap"])
@pytest.mark.parametrize("channels", [1, 3, 4, 5, 8, 11])
def test_channels_and_post(lrp, torch_cuda, channels, post):
    """The run-time channel path, the tonemap on the first min(C, 3) channels of the covered pixels only, and — 11 — a second
    launch for the channels beyond the eighth."""
    scene = Scene(lrp, torch_cuda, cs.OVERLAP_CASES[0], channels=channels, seed=300 + channels)
    for mode, interp in ((cs.FIRST, 2), (cs.MEAN, 1), (cs.FEATHER, 0), (cs.FEATHER, 2)):
        k = scene.check(mode, interp, f"C {channels}", post=post)
    d, _ = scene.compose(cs.FEATHER, 2, post=post, fill=float("nan"))
    torch_cuda.cuda.synchronize()
    got = d.cpu().numpy()
    assert ((got.view(np.uint32) == 0).all(axis=2) == (k == 0)).all(), "an uncovered pixel is +0.0 in every channel, and only it"


def test_no_rotations(lrp, torch_cuda):
    """rotations == NULL: no source is rotated (and no multiplication happens: reproject() without a matrix)."""
    case = cs._case("unrotated", "eqr_full", (96, 48), [("rect18", (64, 48), None), ("rect12", (48, 32), None), ("rect35", (64, 48), None)])
    scene = Scene(lrp, torch_cuda, case, no_rotations=True)
    for mode in cs.MODES:
        k = scene.check(mode, 2, "no rotations")
    assert k.max() == 3 and (k == 0).any()


def test_side_stream(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene(lrp, torch, cs.OVERLAP_CASES[1])
    want, k = scene.expect(cs.FEATHER, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d, plane = scene.compose(cs.FEATHER, 2, count=True, stream=side)
    side.synchronize()
    cases.assert_same_bits(d.cpu().numpy(), want, "side stream")
    assert (plane.cpu().numpy() == k).all()


def test_independent_of_kernel_family_and_geometry_cache(lrp, torch_cuda):
    torch = torch_cuda
    scene = Scene(lrp, torch, cs.OVERLAP_CASES[2])
    want, k = scene.expect(cs.FEATHER, 2)
    lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        im = scene.images()[0]
        d = torch.empty((scene.oh, scene.ow, 4), dtype=torch.float32, device="cuda")
        s0 = lrp.geometry_cache_stats()
        lrp.reproject(im, scene.out_image(d), 1, 2, scene.rot(0))  # the geometry of source 0 enters the cache
        torch.cuda.synchronize()
        s1 = lrp.geometry_cache_stats()
        assert s1["fills"] == s0["fills"] + 1, (s0, s1)
        for cache in (1, 0):
            lrp.debug_set("geo_cache", cache)
            for family in (0, 1, 2, 3):
                lrp.debug_kernel(family)
                got, plane = scene.compose(cs.FEATHER, 2, count=True)
                torch.cuda.synchronize()
                cases.assert_same_bits(got.cpu().numpy(), want, f"kernel family {family}, cache {cache}")
                assert (plane.cpu().numpy() == k).all()
        assert lrp.geometry_cache_stats() == s1, "a compose call moved the cache counters"
    finally:
        lrp.release_cached_tables()


def test_mid_size_cube_by_checksum(lrp, torch_cuda):
    """Six 512^2 faces into 2048 x 1024, bicubic, FEATHER: the checksum (lrp_checksum_device) of the launch's output against that
    of the expectation, composed the same way and uploaded."""
    torch = torch_cuda
    scene = Scene(lrp, torch, cs.CUBE_MID)
    d, plane = scene.compose(cs.FEATHER, 2, count=True)
    torch.cuda.synchronize()
    want, k = scene.expect(cs.FEATHER, 2)
    assert not np.isnan(want).any()
    d_want = torch.from_numpy(want).cuda()
    got_sum, want_sum = lrp.checksums([d, d_want])
    assert got_sum == want_sum
    assert (plane.cpu().numpy() == k).all() and (k == 1).mean() > 0.95 and (k >= 2).any()
