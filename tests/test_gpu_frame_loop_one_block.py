"""-m gpu: the frame-loop window kernels that read the geometry cache render ONE block per wavefront (lrp_win_kernel.h
kOneBlock), whatever "geo_strip" asks for.

A 16-frame reproject_batch that reads the geometry cache must equal, byte for byte, the same 16 frames rendered one launch
each: for every source mode (rectilinear, equidistant, equirect, equirect-loop) and RGB / RGBA / RGBAZ, under geo_strip
1, 2, 4 crossed with batch_frames 3 and 16, at an output size with partial edge blocks (not a multiple of 16) and, for the
rectilinear source, with corner blocks in view (a source narrower than the target).  And rectilinear -> equirect — the one
mapping whose batches keep strips of several blocks unless batch_frames forces the frame loop — with batch_frames 3 and
16, alias pairs on (a full panorama, pan-only rotation) and off (a general rotation)."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True

N_FRAMES = 16
# source mode -> (input lens, input size, output lens, output size, rotation in degrees)
MAPPINGS = {
    "rect": ("rect", (192, 160), "eqd180", (200, 136), (30.0, -15.0, 5.0)),
    "rect_corners": ("rect_tele", (192, 160), "rect", (200, 136), None),  # most of the target lies beyond the source: corner blocks
    "equidistant": ("eqd180", (192, 192), "rect", (200, 136), (30.0, -15.0, 5.0)),
    "equirect": ("eqr_part", (256, 128), "rect", (200, 136), (30.0, -15.0, 5.0)),
    "equirect_loop": ("eqr_full", (256, 128), "rect", (200, 136), (180.0, 0.0, 0.0)),
    "rect_eqr_alias": ("rect", (192, 160), "eqr_full", (256, 136), (30.0, 0.0, 0.0)),
    "rect_eqr_general": ("rect", (192, 160), "eqr_full", (256, 136), (30.0, -15.0, 5.0)),
}
STRIPS, BATCH_FRAMES = (1, 2, 4), (3, 16)


class _Knobs:
    def __init__(self, lrp, values):
        self.lrp, self.values, self.prev = lrp, values, {}

    def __enter__(self):
        self.lrp.release_cached_tables()
        for k, v in self.values.items():
            self.prev[k] = self.lrp.debug_set(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.lrp.debug_set(k, v)
        self.lrp.release_cached_tables()


def _render(lrp, torch, mapping, c, knobs):
    """(single launches, batch) of the 16 frames under `knobs`; the batch is rendered twice — the second one finds the
    geometry-cache entry whatever the first did — and the second result is returned."""
    inp, (iw, ih), out, (ow, oh), deg = MAPPINGS[mapping]
    lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, ow, oh)[out]
    rot = cases.rotation(lrp, deg)
    srcs = []
    for f in range(N_FRAMES):
        t = torch.empty((ih, iw, c), dtype=torch.float32, device="cuda")
        lrp.synth_fill(t, iw, ih, c, 0xF00D0000 + 977 * f, 4 if c == 5 else -1)
        srcs.append(t)
    torch.cuda.synchronize()
    singles = [torch.full((oh, ow, c), -12345.0, dtype=torch.float32, device="cuda") for _ in range(N_FRAMES)]
    with _Knobs(lrp, {"geo_cache": 1}):
        for s, d in zip(srcs, singles):
            lrp.reproject(lrp.Image(lin, iw, ih, c, s), lrp.Image(lout, ow, oh, c, d), 1, 2, rot)
            torch.cuda.synchronize()
    want = [d.cpu().numpy() for d in singles]
    with _Knobs(lrp, dict(knobs, geo_cache=1)):
        for _ in range(2):
            outs = [torch.full((oh, ow, c), -12345.0, dtype=torch.float32, device="cuda") for _ in range(N_FRAMES)]
            lrp.reproject_batch([lrp.Image(lin, iw, ih, c, s) for s in srcs], [lrp.Image(lout, ow, oh, c, d) for d in outs], 1, 2, rot)
            torch.cuda.synchronize()
    return want, [d.cpu().numpy() for d in outs]


def _check(lrp, torch, mapping, c, knobs):
    want, got = _render(lrp, torch, mapping, c, knobs)
    for f, (w, g) in enumerate(zip(want, got)):
        assert w.tobytes() == g.tobytes(), f"{mapping} c={c} {knobs}: frame {f} differs in {int(np.sum(w.view(np.uint32) != g.view(np.uint32)))} words"
    assert any(not np.array_equal(want[0], w) for w in want[1:])  # (the frames are different frames)


@pytest.mark.parametrize("c", [3, 4, 5])
@pytest.mark.parametrize("mapping", ["rect", "rect_corners", "equidistant", "equirect", "equirect_loop"])
def test_batch_equals_single_launches(lrp, torch_cuda, mapping, c):
    _check(lrp, torch_cuda, mapping, c, {})  # the defaults
    for strip in STRIPS:
        for frames in BATCH_FRAMES:
            _check(lrp, torch_cuda, mapping, c, {"geo_strip": strip, "batch_frames": frames})


@pytest.mark.parametrize("c", [3, 4, 5])
@pytest.mark.parametrize("mapping", ["rect_eqr_alias", "rect_eqr_general"])
def test_rect_to_equirect_forced_frame_loop(lrp, torch_cuda, mapping, c):
    for big in (1, 0):  # (the big-window variant has no frame loop: forced, the batch takes the four-wavefront kernels either way)
        for frames in BATCH_FRAMES:
            _check(lrp, torch_cuda, mapping, c, {"batch_frames": frames, "geo_big": big})
            _check(lrp, torch_cuda, mapping, c, {"batch_frames": frames, "geo_big": big, "geo_strip": 2})
