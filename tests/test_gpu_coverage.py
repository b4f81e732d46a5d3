"""GPU: the coverage planes (include/lrp.h "coverage"; csrc/lrp_coverage.hip) against the CPU model (tests/coverage_model.py,
pinned on the CPU by tests/test_coverage.py), byte for byte — all 30 cells with and without a rotation and num_samples 1-4, the
discriminating cases of tests/coverage_cases.py, odd shapes, a misaligned plane between guard bytes, the image mask and the alpha
channel behind a reprojection, independence of the geometry cache and of the kernel family, a context with set_outside (float
and packed 8-bit), the CLI's --mask-outside, and the 4096^2 frame of BASELINE configs[3] against its committed digest."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import cases
import coverage_cases as cc
import coverage_model as model

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True  # (the tests set the cache themselves)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def gpu_plane(lrp, torch, lin, iw, ih, lout, ow, oh, n, rot, **kw):
    plane = lrp.coverage(lrp.Image(lin, iw, ih, 4, None), lrp.Image(lout, ow, oh, 4, None), n, rot, device=0, **kw)
    torch.cuda.synchronize()
    assert plane.dtype == torch.uint8 and tuple(plane.shape) == (oh, ow)
    return plane.cpu().numpy()


def assert_same_plane(got, want, what):
    if not (got == want).all():
        bad = np.argwhere(got != want)
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {want.size} counts differ; first at (x {x}, y {y}): {got[y, x]} vs {want[y, x]}")


CELLS = cc.cells()


@pytest.mark.parametrize("cell", CELLS, ids=[f"{o}<-{s}" for o, s, _ in CELLS])
def test_cells(lrp, torch_cuda, cell):
    out_name, src_name, (iw, ih) = cell
    ow, oh = 80, 48
    lin, lout = cc.lens(lrp, src_name, iw, ih), cc.lens(lrp, out_name, ow, oh)
    seen = set()
    for deg in cc.CELL_ROTATIONS:
        rot = cases.rotation(lrp, deg)
        for n in (1, 2, 3, 4):
            want = model.coverage(lin, iw, ih, lout, ow, oh, n, rot)
            assert_same_plane(gpu_plane(lrp, torch_cuda, lin, iw, ih, lout, ow, oh, n, rot), want, f"{cell} rot {deg} n {n}")
            seen |= set(np.unique(want).tolist())
    assert len(seen) > 1, "a cell whose planes are one constant checks nothing"


@pytest.mark.parametrize("case", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_discriminating_cases(lrp, torch_cuda, case):
    (iw, ih), (ow, oh), n = case["in_size"], case["out_size"], case["n"]
    lin, lout, rot = cc.lens(lrp, case["inp"], iw, ih), cc.lens(lrp, case["out"], ow, oh), cases.rotation(lrp, case["deg"])
    assert_same_plane(gpu_plane(lrp, torch_cuda, lin, iw, ih, lout, ow, oh, n, rot), model.coverage(lin, iw, ih, lout, ow, oh, n, rot), case["name"])


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (33, 17), (49, 49), (67, 9), (259, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes(lrp, torch_cuda, size):
    """Planes of fewer than four pixels, rows that are no multiple of four (a lane's dword continues in the next row), a NaN
    centre (49 x 49 fisheye targets), a 259-wide row that ends inside a wavefront."""
    ow, oh = size
    iw, ih = 64, 48
    lin = cc.lens(lrp, "rect18", iw, ih)
    rot = cases.rotation(lrp, (25.0, 10.0, 0.0))
    for out_name in ("eqr_full", "eqd_pi", "stg", "rect12"):
        lout = cc.lens(lrp, out_name, ow, oh)
        for n in (1, 3):
            want = model.coverage(lin, iw, ih, lout, ow, oh, n, rot)
            assert_same_plane(gpu_plane(lrp, torch_cuda, lin, iw, ih, lout, ow, oh, n, rot), want, f"{size} {out_name} n {n}")
    if size == (49, 49):  # the centre pixel's ray is NaN: uncovered, whatever surrounds it
        lout, back = cc.lens(lrp, "eqd_pi", ow, oh), cases.rotation(lrp, (180.0, 0.0, 0.0))  # (a fisheye target looks along +z)
        got = gpu_plane(lrp, torch_cuda, lin, iw, ih, lout, ow, oh, 1, back)
        assert got[24, 24] == 0 and got[24, 23] == 1 and got[23, 24] == 1


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_misaligned_plane_and_guard_bytes(lrp, torch_cuda, offset):
    torch = torch_cuda
    iw, ih = 64, 48
    lin = cc.lens(lrp, "rect18", iw, ih)
    for ow, oh in ((33, 17), (80, 48), (5, 1)):
        lout = cc.lens(lrp, "eqr_full", ow, oh)
        n_px = ow * oh
        buf = torch.full((64 + offset + n_px + 64 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        first = (-buf.data_ptr()) % 4 + 64 + offset  # a plane `offset` bytes past a 4-byte boundary, 64 or more guard bytes in front
        view = buf[first:first + n_px]
        assert view.data_ptr() % 4 == offset
        got = lrp.coverage(lrp.Image(lin, iw, ih, 4, None), lrp.Image(lout, ow, oh, 4, None), 2, None, out=view)
        torch.cuda.synchronize()
        assert got.data_ptr() == view.data_ptr()
        host = buf.cpu().numpy()
        assert_same_plane(host[first:first + n_px].reshape(oh, ow), model.coverage(lin, iw, ih, lout, ow, oh, 2, None), f"offset {offset} {ow}x{oh}")
        assert (host[:first] == 0xA5).all() and (host[first + n_px:] == 0xA5).all(), "guard bytes written"


def render(lrp, torch, lin, src, lout, ow, oh, n, interp, rot, post=None):
    h, w, c = src.shape
    d_in = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_out = torch.full((oh, ow, c), -1.0, dtype=torch.float32, device="cuda")
    lrp.reproject(lrp.Image(lin, w, h, c, d_in), lrp.Image(lout, ow, oh, c, d_out), n, interp, rot, post=post)
    return d_out


@pytest.mark.parametrize("post", [None, (2.0, 3.0)], ids=["plain", "tonemap"])
@pytest.mark.parametrize("channels", [1, 3, 4, 5])
def test_image_mask(lrp, torch_cuda, channels, post):
    """reproject, then mask_image: the model's image with +0.0 in every channel exactly where the model's count is 0, the same
    bits elsewhere."""
    torch = torch_cuda
    iw, ih, ow, oh = 64, 48, 96, 48
    lin, lout = cc.lens(lrp, "rect18", iw, ih), cc.lens(lrp, "eqr_full", ow, oh)
    rot = cases.rotation(lrp, cc.GENERAL)
    src = cases.hash_noise(ih, iw, channels, 30 + channels, planted=False) + np.float32(0.25)  # (no zero texel: a zero is the mask's)
    for n, interp in ((1, 2), (2, 1), (3, 0)):
        d_out = render(lrp, torch, lin, src, lout, ow, oh, n, interp, rot, post)
        plane = lrp.coverage(lrp.Image(lin, iw, ih, channels, None), lrp.Image(lout, ow, oh, channels, d_out), n, rot, mask_image=True)
        torch.cuda.synchronize()
        want_plane = model.coverage(lin, iw, ih, lout, ow, oh, n, rot)
        assert_same_plane(plane.cpu().numpy(), want_plane, f"C {channels} n {n}")
        want = model.masked(model.reproject(lin, src, lout, ow, oh, n, interp, rot, post=post), want_plane)
        got = d_out.cpu().numpy()
        cases.assert_same_bits(got, want, f"C {channels} n {n} interp {interp} post {post}")
        assert ((got == 0).all(axis=2) == (want_plane == 0)).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_alpha_channel(lrp, torch_cuda, n):
    torch = torch_cuda
    iw, ih, ow, oh = 64, 48, 96, 48
    lin, lout = cc.lens(lrp, "rect18", iw, ih), cc.lens(lrp, "eqr_full", ow, oh)
    rot = cases.rotation(lrp, cc.GENERAL)
    src = cases.hash_noise(ih, iw, 4, 50 + n)
    want = model.reproject(lin, src, lout, ow, oh, n, 2, rot)
    want_plane = model.coverage(lin, iw, ih, lout, ow, oh, n, rot)
    d_out = render(lrp, torch, lin, src, lout, ow, oh, n, 2, rot)
    lrp.coverage(lrp.Image(lin, iw, ih, 4, None), lrp.Image(lout, ow, oh, 4, d_out), n, rot, alpha_channel=3)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    cases.assert_same_bits(got[..., :3], want[..., :3], "the other channels")
    cases.assert_same_bits(got[..., 3], model.alpha(want_plane, n), "alpha == count * normalize")
    # mask and alpha in one call: the alpha of a masked pixel is +0.0
    d_out = render(lrp, torch, lin, src, lout, ow, oh, n, 2, rot)
    lrp.coverage(lrp.Image(lin, iw, ih, 4, None), lrp.Image(lout, ow, oh, 4, d_out), n, rot, mask_image=True, alpha_channel=3)
    torch.cuda.synchronize()
    both = model.masked(want, want_plane)
    both[..., 3] = model.alpha(want_plane, n)
    cases.assert_same_bits(d_out.cpu().numpy(), both, "mask + alpha")


def test_independent_of_geometry_cache_and_kernel_family(lrp, torch_cuda):
    torch = torch_cuda
    iw, ih, ow, oh = 320, 160, 192, 144
    lin, lout = cc.lens(lrp, "eqr_part", iw, ih), cc.lens(lrp, "rect18", ow, oh)
    rot = cases.rotation(lrp, cc.GENERAL)
    src = cases.hash_noise(ih, iw, 4, 8)
    want = model.coverage(lin, iw, ih, lout, ow, oh, 1, rot)
    assert 0.05 < (want == 0).mean() < 0.95
    assert_same_plane(gpu_plane(lrp, torch, lin, iw, ih, lout, ow, oh, 1, rot), want, "cache off")
    lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        s0 = lrp.geometry_cache_stats()
        render(lrp, torch, lin, src, lout, ow, oh, 1, 2, rot)
        torch.cuda.synchronize()
        s1 = lrp.geometry_cache_stats()
        assert s1["fills"] == s0["fills"] + 1, (s0, s1)
        assert_same_plane(gpu_plane(lrp, torch, lin, iw, ih, lout, ow, oh, 1, rot), want, "after a fill")
        assert lrp.geometry_cache_stats() == s1, "a coverage call moved the cache counters"
        render(lrp, torch, lin, src, lout, ow, oh, 1, 2, rot)
        torch.cuda.synchronize()
        s2 = lrp.geometry_cache_stats()
        assert s2["hits"] >= s1["hits"] + 1, (s1, s2)
        assert_same_plane(gpu_plane(lrp, torch, lin, iw, ih, lout, ow, oh, 1, rot), want, "after a hit")
        for family in (0, 1, 2, 3):
            lrp.debug_kernel(family)
            assert_same_plane(gpu_plane(lrp, torch, lin, iw, ih, lout, ow, oh, 1, rot), want, f"kernel family {family}")
        assert lrp.geometry_cache_stats() == s2, "a coverage call moved the cache counters"
    finally:
        lrp.release_cached_tables()


def test_context_set_outside(lrp, torch_cuda):
    """submit and submit_packed (RGBA8 in and out) with set_outside(mask_image=True): the same run without it, composed with the
    model's mask; set_outside(False, -1) restores today's bytes.  An alpha channel through submit."""
    iw, ih, ow, oh = 96, 64, 96, 48
    lin, lout = cc.lens(lrp, "rect18", iw, ih), cc.lens(lrp, "eqr_full", ow, oh)
    rot = cases.rotation(lrp, cc.GENERAL)
    plane = model.coverage(lin, iw, ih, lout, ow, oh, 1, rot)
    src = cases.hash_noise(ih, iw, 4, 61, planted=False) + np.float32(0.25)
    src8 = np.random.default_rng(62).integers(1, 256, size=(ih, iw, 4), dtype=np.uint8)
    post = (2.0, 4.0)

    def run(ctx):
        out = np.full((oh, ow, 4), -1.0, dtype=np.float32)
        out8 = np.full((oh, ow, 4), 7, dtype=np.uint8)
        ctx.submit(lrp.Image(lin, iw, ih, 4, src), lrp.Image(lout, ow, oh, 4, out), 1, 2, rot, post)
        t = ctx.submit_packed(lrp.Image(lin, iw, ih, 4, None), lrp.PixelFormat.U8_GAMMA, src8, lrp.Image(lout, ow, oh, 4, None),
                              lrp.PixelFormat.U8_GAMMA, out8, 255, 1, 2, rot, post)
        ctx.wait_ticket(t)
        ctx.wait()
        return out, out8

    with lrp.BatchContext(device=0, n_streams=3) as ctx:
        plain, plain8 = run(ctx)
        ctx.set_outside(mask_image=True)
        masked, masked8 = run(ctx)
        ctx.set_outside(False, 3)
        out_a = np.full((oh, ow, 4), -1.0, dtype=np.float32)
        ctx.submit(lrp.Image(lin, iw, ih, 4, src), lrp.Image(lout, ow, oh, 4, out_a), 1, 2, rot, post)
        ctx.wait()
        ctx.set_outside(False, 4)  # a channel the image does not have: that submission fails, nothing is enqueued
        with pytest.raises(lrp.LrpError) as e:
            ctx.submit(lrp.Image(lin, iw, ih, 4, src), lrp.Image(lout, ow, oh, 4, out_a.copy()), 1, 2, rot, post)
        assert e.value.status == lrp.Status.BAD_ARG
        ctx.set_outside(False, -1)
        again, again8 = run(ctx)
    assert (plain8[plane > 0] != 0).any() and (plain[plane == 0] != 0).any()
    cases.assert_same_bits(masked, model.masked(plain, plane), "submit")
    want8 = plain8.copy()
    want8[plane == 0] = 0
    assert (masked8 == want8).all(), "submit_packed"
    want_a = plain.copy()
    want_a[..., 3] = model.alpha(plane, 1)
    cases.assert_same_bits(out_a, want_a, "alpha through submit")
    cases.assert_same_bits(again, plain, "set_outside(0, -1)")
    assert (again8 == plain8).all()


def test_cli_mask_outside_png(lrp, torch_cuda, tmp_path):
    from PIL import Image

    cli = os.path.join(os.path.dirname(lrp.__file__), "bin", "reproject")
    w, h, ow, oh = 96, 64, 128, 64
    rgb = np.random.default_rng(31).integers(1, 256, size=(h, w, 3), dtype=np.uint8)
    Image.fromarray(rgb, "RGB").save(tmp_path / "view.png")
    base = [cli, "--single", str(tmp_path / "view.png"), "--png", "--no-configs", f"{w},{h}", "--i-rectilinear", "18,36",
            "--equirectangular", "full", "--output-resolution", f"{ow},{oh}", "--rotation", "20,10,0"]
    for out_dir, extra in (("plain", []), ("masked", ["--mask-outside"])):
        r = subprocess.run(base + ["-o", str(tmp_path / out_dir)] + extra, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    plain = np.array(Image.open(tmp_path / "plain" / "view.png"))
    masked = np.array(Image.open(tmp_path / "masked" / "view.png"))
    d2r = lambda d: float(np.float32(d / 180.0 * np.pi))  # noqa: E731
    rot = lrp.rotation_matrix(d2r(20.0), d2r(10.0), d2r(0.0))
    plane = model.coverage(cc.lens(lrp, "rect18", w, h), w, h, cc.lens(lrp, "eqr_full", ow, oh), ow, oh, 1, rot)
    assert plain.shape == (oh, ow, 4) and 0.05 < (plane == 0).mean() < 0.95 and (plain[plane == 0][:, :3] != 0).any()
    want = plain.copy()
    want[plane == 0, :3] = 0  # (the alpha byte is save_png's fill, not a channel of the image)
    assert (masked == want).all()


def test_full_frame_digest(lrp, torch_cuda):
    """BASELINE configs[3] at 4096 x 4096 against the committed digest of the model's plane."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "coverage_golden.json")))["frame"]
    case = cc.FULL_FRAME
    (iw, ih), (ow, oh) = case["in_size"], case["out_size"]
    got = gpu_plane(lrp, torch_cuda, cc.lens(lrp, case["inp"], iw, ih), iw, ih, cc.lens(lrp, case["out"], ow, oh), ow, oh, case["n"],
                    cases.rotation(lrp, case["deg"]))
    assert int((got == 0).sum()) == golden["count0"] and int((got == case["n"] ** 2).sum()) == golden["count_full"]
    assert hashlib.sha256(got.tobytes()).hexdigest() == golden["sha256"]
