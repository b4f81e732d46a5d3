"""-m gpu: whole frames of the stereographic lens extension against COMMITTED digests (tests/golden/stereographic_golden.json,
written by tests/golden/make_stereographic_golden.py from the CPU model; no model call here): the little planet (a full
4096 x 2048 panorama into one 2048^2 stereographic frame, pitch 90 degrees) and the configs[1] twin, through the launch that
fills the geometry cache, the launch that reads it, the cache off, the one-pixel-per-lane and tile kernel families, and a
16-frame batch."""
import json
import os

import pytest

import cases
import fullframe_cases as ffc
import stereographic_cases as stc

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "stereographic_golden.json")) as _f:
    GOLDEN = json.load(_f)["frames"]


@pytest.fixture(autouse=True)
def ext_on(lrp, torch_cuda):
    prev = lrp.lens_extensions(lrp.LENS_EXT_STEREOGRAPHIC)
    prev_cache = lrp.debug_set("geo_cache", 1)
    lrp.geometry_cache_configure(1 << 30, 1)
    lrp.release_cached_tables()
    try:
        yield
    finally:
        lrp.debug_set("geo_cache", prev_cache)
        lrp.release_cached_tables()
        lrp.lens_extensions(prev)


def _setup(lrp, torch, case):
    (iw, ih), (ow, oh), c = case["in_size"], case["out_size"], case["c"]
    d_in = torch.empty((ih, iw, c), dtype=torch.float32, device="cuda")
    lrp.synth_fill(d_in, iw, ih, c, case["seed"], case["depth"])
    lin, lout = stc.lens(lrp, case["inp"], iw, ih), stc.lens(lrp, case["out"], ow, oh)
    return d_in, lrp.Image(lin, iw, ih, c, d_in), lout


def _check(d_out, name, what):
    want = GOLDEN[name]
    sha, bands, n_nan = ffc.frame_digests(d_out.cpu().numpy())
    bad = [b for b in range(ffc.BANDS) if bands[b] != want["bands"][b]]
    assert not bad, f"{name} ({what}): row bands {bad} of {ffc.BANDS} differ from the committed digest"
    assert sha == want["sha256"] and n_nan == want["nan"], f"{name} ({what})"


def test_golden_holds_the_issue_cases():
    assert sorted(GOLDEN) == sorted(stc.frame_cases())
    assert "stg_little_planet_eqr_stg_bc" in GOLDEN and "stg_config1_4k_stg_rect_bc" in GOLDEN


@pytest.mark.parametrize("name", sorted(stc.frame_cases()))
def test_whole_frame_equals_committed_digest(lrp, torch_cuda, name):
    torch = torch_cuda
    case = stc.frame_cases()[name]
    assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in case.items() if k != "name"} == GOLDEN[name]["case"], \
        "fixture was generated for another case definition: re-run tests/golden/make_stereographic_golden.py"
    (ow, oh), c = case["out_size"], case["c"]
    d_in, im_in, lout = _setup(lrp, torch, case)
    rot = cases.rotation(lrp, case["deg"])
    post = tuple(case["post"]) if case["post"] else None
    d_out = torch.empty((oh, ow, c), dtype=torch.float32, device="cuda")

    def render(what):
        d_out.fill_(-12345.0)
        lrp.reproject(im_in, lrp.Image(lout, ow, oh, c, d_out), 1, case["interp"], rot, post=post)
        torch.cuda.synchronize()
        _check(d_out, name, what)

    s0 = lrp.geometry_cache_stats()
    render("filling launch")
    s1 = lrp.geometry_cache_stats()
    assert s1["fills"] == s0["fills"] + 1, (s0, s1)
    render("reading launch")
    assert lrp.geometry_cache_stats()["hits"] >= s1["hits"] + 1
    lrp.debug_set("geo_cache", 0)
    render("cache off")
    for family in (0, 1):
        prev = lrp.debug_kernel(family)
        try:
            render(f"kernel family {family}")
        finally:
            lrp.debug_kernel(prev)


@pytest.mark.parametrize("cache", [0, 1])
def test_batch_of_16_equals_committed_digest(lrp, torch_cuda, cache):
    """The configs[1] twin as bench.py renders a directory: 16 frames of one geometry per launch (every frame the same source
    here, so each must equal the committed frame)."""
    torch = torch_cuda
    lrp.debug_set("geo_cache", cache)
    name = "stg_config1_4k_stg_rect_bc"
    case = stc.frame_cases()[name]
    (ow, oh), c = case["out_size"], case["c"]
    d_in, im_in, lout = _setup(lrp, torch, case)
    d_outs = [torch.full((oh, ow, c), -12345.0, dtype=torch.float32, device="cuda") for _ in range(16)]
    lrp.reproject_batch([im_in] * 16, [lrp.Image(lout, ow, oh, c, d) for d in d_outs], 1, case["interp"], None)
    torch.cuda.synchronize()
    for i in (0, 1, 7, 15):
        _check(d_outs[i], name, f"batch frame {i}, cache {cache}")
