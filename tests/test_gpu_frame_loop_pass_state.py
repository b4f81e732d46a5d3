"""-m gpu: the one-block frame-loop window kernels hold a pass's lane state — weights, window address, destination offset —
across the frames of a launch (lrp_win_kernel.h PassLane, kHoist) instead of deriving it from the coordinates in every pass
of every frame.  The state is a matter of the geometry alone, so nothing may change in the output.

A batch rendered by the frame loop (batch_frames 16: a wavefront walks up to 16 frames of its block) must equal, bit for
bit (numpy.array_equal on the raw words), the same frames rendered by single-frame launches (batch_frames 1: the
instantiations without the frame loop, which derive everything per pass).  Mappings, chosen so that every tier of these
kernels has blocks in view:
  coefficient tier   magnified views: fisheye -> rectilinear, partial panorama -> rectilinear
  raw-tap tier       about 1:1: rectilinear -> rectilinear under a small rotation (the planes of a block do not fit)
  gathers            a view minified about three times (no window fits: the held state is the coordinates themselves)
  edge row / edge column / corner blocks   a tele source inside a wider rectilinear target: the blocks above / below, left /
                     right of and diagonally beyond the source
Blocks per tier when this test was written (a -DLRP_TIER_STATS build, RGBA, the counters tools/tier_census.py reads;
profiles/r08_frame_loop_pass_state.txt), so that a change of the planner's thresholds that empties a tier can be seen:
  eqd_eqd_minified      raw 1, gathers 63                         eqd_rect_magnified   coefficient 117
  eqr_loop_rect         coefficient 108, gathers 9                eqr_rect_magnified   coefficient 23, raw 44, gathers 49, corner 1
  rect_rect_1to1        coefficient 12, raw 91, gathers 14        tele_in_wide         gathers 56, corner 28, edge row 12, edge column 21
  tele_in_wide_rolled   gathers 49, corner 35, edge row 13, edge column 20
RGB, RGBA, and RGBAZ with and without the fused tonemap; batches of 1, 5 and 16 frames (1: a single launch; 5: a frame
loop that ends early); output sizes that are not multiples of 16, where the lanes beyond the image store the clamped pixel
a second time."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True

# name -> (input lens, input size, output lens, output size, rotation in degrees)
MAPPINGS = {
    "eqd_rect_magnified": ("eqd180", (192, 192), "rect", (200, 136), (30.0, -15.0, 5.0)),
    "eqr_rect_magnified": ("eqr_part", (256, 128), "rect", (203, 131), (30.0, -15.0, 5.0)),
    "eqr_loop_rect": ("eqr_full", (256, 128), "rect", (200, 136), (180.0, 0.0, 0.0)),
    "rect_rect_1to1": ("rect", (208, 144), "rect", (203, 131), (2.0, -1.0, 3.0)),
    "eqd_eqd_minified": ("eqd180", (384, 384), "eqd180", (120, 117), (10.0, 5.0, 0.0)),
    "tele_in_wide": ("rect_tele", (192, 160), "rect", (200, 136), None),
    "tele_in_wide_rolled": ("rect_tele", (192, 160), "rect", (203, 131), (0.0, 0.0, 1.0)),
}
CHANNELS_POST = [(3, None), (4, None), (5, None), (5, (2.0, 3.0)), (4, (2.0, 3.0))]
BATCHES = (1, 5, 16)


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


def _batch(lrp, torch, mapping, c, post, n, knobs):
    """The n frames rendered as one reproject_batch under `knobs`, twice: the second call finds the geometry-cache entry
    (the launches that read it are the ones under test) and its result is returned."""
    inp, (iw, ih), out, (ow, oh), deg = MAPPINGS[mapping]
    lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, ow, oh)[out]
    rot = cases.rotation(lrp, deg)
    srcs = []
    for f in range(n):
        t = torch.empty((ih, iw, c), dtype=torch.float32, device="cuda")
        lrp.synth_fill(t, iw, ih, c, 0xBEE50000 + 977 * f, 4 if c == 5 else -1)
        srcs.append(t)
    torch.cuda.synchronize()
    with _Knobs(lrp, dict(knobs, geo_cache=1)):
        for _ in range(2):
            outs = [torch.full((oh, ow, c), -12345.0, dtype=torch.float32, device="cuda") for _ in range(n)]
            lrp.reproject_batch([lrp.Image(lin, iw, ih, c, s) for s in srcs], [lrp.Image(lout, ow, oh, c, d) for d in outs], 1, 2, rot,
                                post=post)
            torch.cuda.synchronize()
    return [d.cpu().numpy() for d in outs]


@pytest.mark.parametrize("c,post", CHANNELS_POST)
@pytest.mark.parametrize("mapping", sorted(MAPPINGS))
def test_frame_loop_equals_single_frame_launches(lrp, torch_cuda, mapping, c, post):
    for n in BATCHES:
        want = _batch(lrp, torch_cuda, mapping, c, post, n, {"batch_frames": 1})
        for knobs in ({"batch_frames": 16}, {}):  # the frame loop forced to its full length, and the launcher's own choice
            got = _batch(lrp, torch_cuda, mapping, c, post, n, knobs)
            for f, (w, g) in enumerate(zip(want, got)):
                wb, gb = w.view(np.uint32), g.view(np.uint32)
                assert np.array_equal(wb, gb), f"{mapping} c={c} post={post} n={n} {knobs}: frame {f} differs in {int(np.sum(wb != gb))} words"
        assert not np.any(want[0] == np.float32(-12345.0))  # (every pixel was written)
        if n > 1:
            assert any(not np.array_equal(want[0], w) for w in want[1:])  # (the frames are different frames)
