"""GPU: the stereographic fisheye lens extension (include/lrp.h LRP_LENS_EXT_STEREOGRAPHIC) against the CPU model
(tests/stereographic_model.py, its loop pinned to the oracle) bit for bit, any NaN equal to any NaN — the ten stereographic
cells (the two shared with the equisolid lens included) x the three samplers x rotations through every kernel family,
channels 1-5, odd and even sizes, num_samples 1-4, the fused tonemap, the geometry cache (the filling launch, the reading
launch, off), a row band, batches of 16 and 17, multi_device, a context's packed path, a graph capture, and the CLI with and
without --allow-stereographic.  Every test switches the extension on and back off (the rejection tests share the process)."""
import math

import numpy as np
import pytest

import cases
import stereographic_model as model

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True  # (the tests set the cache themselves)



@pytest.fixture(autouse=True)
def ext_on(lrp, torch_cuda):
    prev = lrp.lens_extensions(lrp.LENS_EXT_STEREOGRAPHIC)
    prev_cache = lrp.debug_set("geo_cache", 0)
    prev_kernel = lrp.debug_kernel(-1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        yield
    finally:
        lrp.debug_kernel(prev_kernel)
        lrp.debug_set("geo_cache", prev_cache)
        lrp.release_cached_tables()
        lrp.lens_extensions(prev)


def lens_set(lrp, w, h):
    """name -> lens for an image of w x h: stereographic lenses, the README's equisolid lens and the reference's lenses."""
    return {
        "stg": lrp.LensInfo.stereographic(12.5, 36.0, w, h),
        "stg_wide": lrp.LensInfo.stereographic(4.0, 36.0, w, h),  # the frame's edge at theta = 132 degrees
        "eqs": lrp.LensInfo.equisolid(12.5, 36.0, math.pi, w, h),
        "eqs_narrow": lrp.LensInfo.equisolid(20.0, 36.0, 2.0, w, h),
        "rect": lrp.LensInfo.rectilinear(18.0, 36.0, w, h),
        "eqd": lrp.LensInfo.equidistant(math.pi),
        "eqr_full": lrp.LensInfo.equirectangular(),
        "eqr_part": lrp.LensInfo.equirectangular(-1.0, 1.5, -0.6, 0.7),
    }


# the ten cells: (output lens, source lens) — a stereographic target with the six source modes, the four other targets with a
# stereographic source
CELLS = [("stg", "rect"), ("stg", "eqd"), ("stg", "eqr_part"), ("stg", "eqr_full"), ("stg", "eqs"), ("stg_wide", "stg"),
         ("rect", "stg"), ("eqd", "stg"), ("eqs", "stg"), ("eqr_part", "stg")]
ROTS = [None, (0.0, 0.0, 0.0), (30.0, -15.0, 5.0)]


def render(lrp, torch, lin, src, lout, ow, oh, ns, interp, rot, post=None):
    h, w, c = src.shape
    d_in = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    d_out = torch.full((oh, ow, c), -1.0, dtype=torch.float32, device="cuda")
    lrp.reproject(lrp.Image(lin, w, h, c, d_in), lrp.Image(lout, ow, oh, c, d_out), ns, interp, rot, post=post)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("cell", CELLS, ids=[f"{o}<-{i}" for o, i in CELLS])
def test_cells_samplers_rotations_families(lrp, torch_cuda, cell):
    torch = torch_cuda
    iw, ih, ow, oh = 67, 45, 41, 33
    src = cases.hash_noise(ih, iw, 4, 11)
    lin, lout = lens_set(lrp, iw, ih)[cell[1]], lens_set(lrp, ow, oh)[cell[0]]
    if "eqs" in cell:  # a cell shared with the equisolid lens needs both bits (the fixture restores the mask)
        a = np.zeros((4, 4, 4), dtype=np.float32)
        with pytest.raises(lrp.LrpError):
            lrp.reproject(lrp.Image(lin, 4, 4, 4, a), lrp.Image(lout, 4, 4, 4, a.copy()), 1, 0)
        lrp.lens_extensions(lrp.LENS_EXT_STEREOGRAPHIC | lrp.LENS_EXT_EQUISOLID)
    for rot_deg in ROTS:
        rot = cases.rotation(lrp, rot_deg)
        for interp in (0, 1, 2):
            want = model.reproject(lin, src, lout, ow, oh, 1, interp, rot)
            for family in (0, 1, 2, 3):
                lrp.debug_kernel(family)
                got = render(lrp, torch, lin, src, lout, ow, oh, 1, interp, rot)
                cases.assert_same_bits(got, want, f"{cell} rot {rot_deg} interp {interp} family {family}")


@pytest.mark.parametrize("channels", [1, 2, 3, 4, 5])
def test_channels_sizes_and_supersampling(lrp, torch_cuda, channels):
    torch = torch_cuda
    rot = cases.rotation(lrp, (30.0, -15.0, 5.0))
    for (iw, ih, ow, oh) in ((64, 48, 40, 32), (61, 47, 39, 31)):
        src = cases.hash_noise(ih, iw, channels, channels)
        for cell in (("stg_wide", "eqr_full"), ("rect", "stg"), ("stg", "stg_wide")):
            lin, lout = lens_set(lrp, iw, ih)[cell[1]], lens_set(lrp, ow, oh)[cell[0]]
            for interp in (0, 1, 2):
                for ns in (1, 2, 3, 4):
                    want = model.reproject(lin, src, lout, ow, oh, ns, interp, rot)
                    got = render(lrp, torch, lin, src, lout, ow, oh, ns, interp, rot)
                    cases.assert_same_bits(got, want, f"C {channels} {iw}x{ih} {cell} interp {interp} ns {ns}")


def test_post_process(lrp, torch_cuda):
    lin, lout = lens_set(lrp, 96, 64)["eqr_full"], lens_set(lrp, 48, 48)["stg"]
    src = cases.hash_noise(64, 96, 5, 2)
    want = model.reproject(lin, src, lout, 48, 48, 1, 2, None, post=(2.0, 3.0))
    cases.assert_same_bits(render(lrp, torch_cuda, lin, src, lout, 48, 48, 1, 2, None, post=(2.0, 3.0)), want, "post")


@pytest.mark.parametrize("interp,ns", [(2, 1), (1, 1), (0, 1), (1, 2), (2, 3)])
def test_geometry_cache_fill_then_hit(lrp, torch_cuda, interp, ns):
    """The first launch of a geometry computes and writes the entry; the second reads it (the existing lens-agnostic
    GeoRead kernels); both equal the model; then the same with the cache off."""
    torch = torch_cuda
    lrp.debug_set("geo_cache", 1)
    iw, ih, ow, oh = 320, 160, 192, 144
    lin, lout = lens_set(lrp, iw, ih)["eqr_full"], lens_set(lrp, ow, oh)["stg"]
    rot = cases.rotation(lrp, (30.0, -15.0, 5.0))
    for cell in ((lin, lout), (lens_set(lrp, iw, ih)["stg"], lens_set(lrp, ow, oh)["rect"])):
        lrp.release_cached_tables()
        s0 = lrp.geometry_cache_stats()
        for k, seed in enumerate((1, 2)):
            src = cases.hash_noise(ih, iw, 4, seed)
            want = model.reproject(cell[0], src, cell[1], ow, oh, ns, interp, rot)
            cases.assert_same_bits(render(lrp, torch, cell[0], src, cell[1], ow, oh, ns, interp, rot), want, f"call {k}")
            s = lrp.geometry_cache_stats()
            if k == 0:
                assert s["fills"] == s0["fills"] + 1, (s0, s)
            else:
                assert s["hits"] >= s0["hits"] + 1, (s0, s)
    lrp.debug_set("geo_cache", 0)
    src = cases.hash_noise(ih, iw, 4, 3)
    want = model.reproject(lin, src, lout, ow, oh, ns, interp, rot)
    cases.assert_same_bits(render(lrp, torch, lin, src, lout, ow, oh, ns, interp, rot), want, "cache off")


def test_row_band(lrp, torch_cuda):
    torch = torch_cuda
    iw, ih, ow, oh = 128, 64, 80, 72
    lin, lout = lens_set(lrp, iw, ih)["eqr_full"], lens_set(lrp, ow, oh)["stg"]
    src = cases.hash_noise(ih, iw, 4, 4)
    for interp in (0, 1, 2):
        want = model.reproject(lin, src, lout, ow, oh, 1, interp, None)
        d_in = torch.from_numpy(src).cuda()
        d_out = torch.full((oh, ow, 4), -1.0, dtype=torch.float32, device="cuda")
        lrp.reproject_rows(lrp.Image(lin, iw, ih, 4, d_in), lrp.Image(lout, ow, oh, 4, d_out), 1, interp, 13, 29)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        cases.assert_same_bits(got[13:42], want[13:42], f"band interp {interp}")
        assert (got[:13] == -1.0).all() and (got[42:] == -1.0).all()


@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("cache", [0, 1])
def test_batches(lrp, torch_cuda, n, cache):
    torch = torch_cuda
    lrp.debug_set("geo_cache", cache)
    iw, ih, ow, oh = 96, 64, 64, 48
    lin, lout = lens_set(lrp, iw, ih)["stg"], lens_set(lrp, ow, oh)["eqd"]
    rot = cases.rotation(lrp, (30.0, -15.0, 5.0))
    for interp in (2, 1, 0):
        srcs = [cases.hash_noise(ih, iw, 4, 100 + i, planted=False) for i in range(n)]
        d_ins = [torch.from_numpy(s).cuda() for s in srcs]
        d_outs = [torch.full((oh, ow, 4), -1.0, dtype=torch.float32, device="cuda") for _ in range(n)]
        lrp.reproject_batch([lrp.Image(lin, iw, ih, 4, d) for d in d_ins], [lrp.Image(lout, ow, oh, 4, d) for d in d_outs], 1, interp, rot)
        torch.cuda.synchronize()
        for i in range(n):
            cases.assert_same_bits(d_outs[i].cpu().numpy(), model.reproject(lin, srcs[i], lout, ow, oh, 1, interp, rot),
                                   f"frame {i} interp {interp}")


def test_multi_device(lrp, torch_cuda):
    torch = torch_cuda
    iw, ih = 128, 64
    src = cases.hash_noise(ih, iw, 4, 5)
    lin = lens_set(lrp, iw, ih)["eqr_full"]
    outs = [(lens_set(lrp, 48, 40)["stg"], 48, 40), (lens_set(lrp, 33, 31)["stg_wide"], 33, 31), (lens_set(lrp, 40, 40)["rect"], 40, 40)]
    rots = np.stack([np.asarray(cases.rotation(lrp, d), dtype=np.float32).reshape(9) for d in ((10, 0, 0), (30, -15, 5), (0, 20, 0))])
    d_in = torch.from_numpy(src).cuda()
    d_outs = [torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda") for _, w, h in outs]
    lrp.reproject_multi(lrp.Image(lin, iw, ih, 4, d_in), [lrp.Image(l, w, h, 4, d) for (l, w, h), d in zip(outs, d_outs)], 1, 2, rots)
    torch.cuda.synchronize()
    for k, ((l, w, h), d) in enumerate(zip(outs, d_outs)):
        cases.assert_same_bits(d.cpu().numpy(), model.reproject(lin, src, l, w, h, 1, 2, rots[k]), f"output {k}")


def test_context_submit_packed(lrp, torch_cuda):
    iw, ih, ow, oh = 96, 64, 56, 48
    lin, lout = lens_set(lrp, iw, ih)["stg"], lens_set(lrp, ow, oh)["eqr_part"]
    srcs = [cases.hash_noise(ih, iw, 4, 40 + i, planted=False) for i in range(3)]
    outs = [np.zeros((oh, ow, 4), dtype=np.float32) for _ in srcs]
    with lrp.BatchContext(device=0, n_streams=3) as ctx:
        tickets = [ctx.submit_packed(lrp.Image(lin, iw, ih, 4, None), lrp.PixelFormat.F32, s, lrp.Image(lout, ow, oh, 4, None),
                                     lrp.PixelFormat.F32, o, 0, 1, 1, None) for s, o in zip(srcs, outs)]
        for t in tickets:
            ctx.wait_ticket(t)
        ctx.wait()
    for i, (s, o) in enumerate(zip(srcs, outs)):
        cases.assert_same_bits(o, model.reproject(lin, s, lout, ow, oh, 1, 1, None), f"image {i}")


def test_graph_capture(lrp, torch_cuda):
    torch = torch_cuda
    iw, ih, ow, oh = 128, 64, 64, 64
    lin, lout = lens_set(lrp, iw, ih)["eqr_full"], lens_set(lrp, ow, oh)["stg"]
    rot = cases.rotation(lrp, (30.0, -15.0, 5.0))
    srcs = [cases.hash_noise(ih, iw, 4, 60 + i) for i in range(2)]
    d_in = torch.from_numpy(srcs[0]).cuda()
    d_out = torch.zeros((oh, ow, 4), dtype=torch.float32, device="cuda")
    args = (lrp.Image(lin, iw, ih, 4, d_in), lrp.Image(lout, ow, oh, 4, d_out), 1, 2, rot)
    lrp.reproject(*args)  # (warm-up outside the capture: tables)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lrp.reproject(*args)
    for s in (srcs[1], srcs[0]):
        d_in.copy_(torch.from_numpy(s))
        d_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        cases.assert_same_bits(d_out.cpu().numpy(), model.reproject(lin, s, lout, ow, oh, 1, 2, rot), "graph replay")


def test_same_lens_nearest_is_the_point_mirrored_input(lrp, torch_cuda):
    """Independent of the model: stereographic -> stereographic, the same lens, nearest, no rotation.  The x / -z fold of the
    source side (as for the reference's equidistant lens) maps the ray of pixel (x, y) to the source position of pixel
    (W-1-x, H-1-y): inside the front hemisphere (theta < pi / 2, r_mm < 2 f tan(pi / 4) = 2 f) the output is the input
    mirrored through the centre, exactly."""
    w = h = 96
    lens = lrp.LensInfo.stereographic(12.5, 36.0, w, h)
    src = cases.hash_noise(h, w, 4, 77, planted=False)
    got = render(lrp, torch_cuda, lens, src, lens, w, h, 1, 0, None)
    y, x = np.mgrid[0:h, 0:w]
    r_mm = np.hypot(x + 0.5 - w / 2, y + 0.5 - h / 2) / w * 36.0
    inside = r_mm < 0.98 * 2 * 12.5
    assert inside.sum() > 0.5 * w * h
    cases.assert_same_bits(got[inside], src[::-1, ::-1][inside], "same lens, nearest")


def test_little_planet_every_pixel_is_rendered(lrp, torch_cuda):
    """A full panorama into one stereographic frame, looking at the pole: there is no "beyond the image circle" — no pixel
    of an even-sized output is NaN (finite source), and the frame equals the model."""
    iw, ih, ow, oh = 256, 128, 96, 96
    lin, lout = lens_set(lrp, iw, ih)["eqr_full"], lrp.LensInfo.stereographic(2.0, 36.0, ow, oh)
    src = cases.hash_noise(ih, iw, 4, 9, planted=False)
    rot = cases.rotation(lrp, (0.0, 90.0, 0.0))
    for interp in (0, 1, 2):
        got = render(lrp, torch_cuda, lin, src, lout, ow, oh, 1, interp, rot)
        assert np.isfinite(got).all()
        cases.assert_same_bits(got, model.reproject(lin, src, lout, ow, oh, 1, interp, rot), f"little planet interp {interp}")


def test_cli_allow_stereographic_exr_equals_model(lrp, torch_cuda, tmp_path):
    import subprocess

    import exr_util

    cli = lrp.__file__.rsplit("/", 1)[0] + "/bin/reproject"
    rng = np.random.default_rng(23)
    w, h = 80, 60
    ch = {n: rng.random((h, w)).astype(np.float16) for n in "RGBA"}
    exr_util.write_exr(str(tmp_path / "pano.exr"), ch, 2)
    base = [cli, "--single", str(tmp_path / "pano.exr"), "-o", str(tmp_path / "o"), "--exr", "--no-configs", f"{w},{h}",
            "--i-equirectangular", "full", "--stereographic", "12.5,36"]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 1 and "Output lens type not supported." in r.stdout  # (off by default)
    r = subprocess.run(base + ["--allow-equisolid"], capture_output=True, text=True)
    assert r.returncode == 1 and "Output lens type not supported." in r.stdout  # (the other extension does not admit it)
    r = subprocess.run(base + ["--allow-stereographic"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    src = np.stack([ch[n].astype(np.float32) for n in "RGBA"], axis=2)
    lout = lrp.LensInfo.stereographic(12.5, 36.0, w, h)
    want = model.reproject(lrp.LensInfo.equirectangular(), src, lout, w, h, 1, 2, lrp.rotation_matrix(0.0, 0.0, 0.0))
    back = exr_util.read_exr(str(tmp_path / "o" / "pano.exr"))
    for i, n in enumerate("RGBA"):
        w16 = want[..., i].astype(np.float16)
        assert ((back[n].view(np.uint16) == w16.view(np.uint16)) | (np.isnan(back[n]) & np.isnan(w16))).all(), n


def test_cli_allow_stereographic_png_equals_model_pipeline(lrp, torch_cuda, tmp_path):
    """PNG in, PNG out (the packed 8-bit path: decode, reproject, tonemap and quantise on the device) out of a stereographic
    frame, against the model with the reference's host decode / post_process / quantiser; without the flag: exit 1 with the
    reference's message."""
    import subprocess

    from PIL import Image

    import test_cli

    cli = lrp.__file__.rsplit("/", 1)[0] + "/bin/reproject"
    rng = np.random.default_rng(29)
    w, h, ow, oh = 96, 64, 64, 48
    rgb = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    Image.fromarray(rgb, "RGB").save(tmp_path / "fish.png")
    base = [cli, "--single", str(tmp_path / "fish.png"), "-o", str(tmp_path / "out"), "--png", "--no-configs", f"{w},{h}",
            "--i-stereographic", "12.5,36", "--rectilinear", "18,36", "--output-resolution", f"{ow},{oh}",
            "--rotation", "10,5,0", "--exposure", "1", "--reinhard", "4"]
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 1 and "Input lens type not supported." in r.stdout
    r = subprocess.run(base + ["--allow-stereographic"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lin = lrp.LensInfo.stereographic(12.5, 36.0, w, h)
    lout = lrp.LensInfo.rectilinear(18.0, 36.0, ow, oh)
    d2r = lambda d: float(np.float32(d / 180.0 * math.pi))  # noqa: E731
    rot = lrp.rotation_matrix(d2r(10.0), d2r(5.0), d2r(0.0))
    want = model.reproject(lin, test_cli.DECODE[rgb], lout, ow, oh, 1, 2, rot, post=(float(np.float32(2.0)), 4.0))
    got = np.array(Image.open(tmp_path / "out" / "fish.png"))
    assert got.shape == (oh, ow, 4) and (got[..., 3] == 255).all()
    assert (got[..., :3] == test_cli.encode8(want)).all()
