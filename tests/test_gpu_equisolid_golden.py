"""-m gpu: whole 4096^2 frames of the equisolid lens extension against COMMITTED digests (tests/golden/equisolid_golden.json,
written by tests/golden/make_equisolid_golden.py from the CPU model; no model call here): the configs[1] / configs[2] twins and
RGBAZ + tonemap into a panorama, through the launch that fills the geometry cache, the launch that reads it, the cache off,
the one-pixel-per-lane and tile kernel families, and a 16-frame batch."""
import json
import os

import pytest

import cases
import equisolid_cases as eqc
import fullframe_cases as ffc

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "equisolid_golden.json")) as _f:
    GOLDEN = json.load(_f)["frames"]


@pytest.fixture(autouse=True)
def ext_on(lrp, torch_cuda):
    prev = lrp.lens_extensions(lrp.LENS_EXT_EQUISOLID)
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
    n, m, c = case["size"], case["out_size"], case["c"]
    d_in = torch.empty((n, n, c), dtype=torch.float32, device="cuda")
    lrp.synth_fill(d_in, n, n, c, case["seed"], case["depth"])
    lin, lout = eqc.lens(lrp, case["inp"], n, n), eqc.lens(lrp, case["out"], m, m)
    return d_in, lrp.Image(lin, n, n, c, d_in), lout


def _check(d_out, name, what):
    want = GOLDEN[name]
    sha, bands, n_nan = ffc.frame_digests(d_out.cpu().numpy())
    bad = [b for b in range(ffc.BANDS) if bands[b] != want["bands"][b]]
    assert not bad, f"{name} ({what}): row bands {bad} of {ffc.BANDS} differ from the committed digest"
    assert sha == want["sha256"] and n_nan == want["nan"], f"{name} ({what})"


@pytest.mark.parametrize("name", sorted(eqc.frame_cases()))
def test_whole_frame_equals_committed_digest(lrp, torch_cuda, name):
    torch = torch_cuda
    case = eqc.frame_cases()[name]
    assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in case.items() if k != "name"} == GOLDEN[name]["case"], \
        "fixture was generated for another case definition: re-run tests/golden/make_equisolid_golden.py"
    m, c = case["out_size"], case["c"]
    d_in, im_in, lout = _setup(lrp, torch, case)
    rot = cases.rotation(lrp, case["deg"])
    post = tuple(case["post"]) if case["post"] else None
    d_out = torch.empty((m, m, c), dtype=torch.float32, device="cuda")

    def render(what):
        d_out.fill_(-12345.0)
        lrp.reproject(im_in, lrp.Image(lout, m, m, c, d_out), 1, case["interp"], rot, post=post)
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
    """configs[1] twin as bench.py renders a directory: 16 frames of one geometry per launch (every frame the same source here,
    so each must equal the committed frame)."""
    torch = torch_cuda
    lrp.debug_set("geo_cache", cache)
    name = "eqs_config1_4k_eqs_rect_bc"
    case = eqc.frame_cases()[name]
    m, c = case["out_size"], case["c"]
    d_in, im_in, lout = _setup(lrp, torch, case)
    d_outs = [torch.full((m, m, c), -12345.0, dtype=torch.float32, device="cuda") for _ in range(16)]
    lrp.reproject_batch([im_in] * 16, [lrp.Image(lout, m, m, c, d) for d in d_outs], 1, case["interp"], None)
    torch.cuda.synchronize()
    for i in (0, 1, 7, 15):
        _check(d_outs[i], name, f"batch frame {i}, cache {cache}")
