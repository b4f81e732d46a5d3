"""-m gpu: the one-block frame-loop window kernels dispatch on the tier of their block once, in front of the frame loop
(lrp_win_kernel.h frame_loop_tier_dispatch): a block of the coefficient tier runs a frame loop of its own (coef_frames: the
wait, precompute(), four passes, the request of the next frame's window with the pointers fetched a frame ahead), every other
tier the generic loop, compiled without the coefficient tier.  What a pass reads and computes is untouched, so the rendered
words must be the oracle's, bit for bit, for every tier on either side of the dispatch.

Mappings: the seven of tests/test_gpu_lds_lane_map.py at 40 x 36 with sources of about 64 x 64 (coefficient, raw taps,
gathers and corner blocks, different tiers in one launch; blocks per tier: that file's docstring), the edge-tier mapping of
tests/test_gpu_frame_loop_pass_state.py at 200 x 136 (tele_in_wide: gathers 56, corner 28, edge row 12, edge column 21), and
half_block_planes, a magnified view of a partial panorama chosen on the CPU with the plan model of
tools/analysis/lds_conflict_census.py (RGB / RGBA windows) for a coefficient block whose planes fit per half only (`whole`
clear), so that the second precompute() of the new loop runs: of its nine blocks, coefficient with whole-block planes 2,
coefficient with half-block planes 1, raw taps 1, nothing staged (gathers / corner) 5
(tests/test_frame_loop_half_planes_plan.py asserts that split on the CPU, so that a changed threshold cannot empty it unseen).
RGB, RGBA, RGBAZ, and RGBAZ with the fused tonemap (the tonemap branch behind the new loop).  Batches of 1, 2, 3 and 16 frames
through reproject_batch: 1 is a single launch without the frame loop, 2 a loop that ends at once, 3 has a middle frame with
a predecessor and a successor (its pointers were fetched a frame ahead and it fetches the next one's), 16 the full count.
Under batch_frames 16 and under the launcher's own choice of frames per wavefront; every batch is rendered twice, so that the
second call reads the geometry cache (the launches under test)."""
import numpy as np
import pytest

import cases
import oracle_binding as oracle

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True

# name -> (input lens, input size, output lens, output size, rotation in degrees)
MAPPINGS = {
    "eqd_rect_magnified": ("eqd180", (56, 56), "rect", (40, 36), (30.0, -15.0, 5.0)),
    "eqr_rect_magnified": ("eqr_part", (64, 32), "rect", (40, 36), (30.0, -15.0, 5.0)),
    "eqr_loop_rect": ("eqr_full", (80, 40), "rect", (40, 36), (180.0, 0.0, 0.0)),
    "rect_rect_1to1": ("rect", (52, 56), "rect", (40, 36), (2.0, -1.0, 3.0)),
    "eqd_eqd_minified": ("eqd180", (128, 128), "eqd180", (40, 36), (10.0, 5.0, 0.0)),
    "tele_in_wide": ("rect_tele", (64, 56), "rect", (40, 36), None),
    "tele_in_wide_rolled": ("rect_tele", (64, 56), "rect", (40, 36), (0.0, 0.0, 1.0)),
    "tele_in_wide_edges": ("rect_tele", (192, 160), "rect", (200, 136), None),
    "half_block_planes": ("eqr_part", (40, 40), "rect", (40, 36), (30.0, -15.0, 5.0)),
}
CHANNELS_POST = [(3, None), (4, None), (5, None), (5, (2.0, 3.0))]
BATCHES = (1, 2, 3, 16)
N_FRAMES = max(BATCHES)


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


_reference = {}


def _frames_and_oracle(lrp, mapping, c, post):
    """The 16 source frames of (mapping, c) and the oracle's rendering of each (with `post`: tonemapped by the oracle):
    computed once, shared, read-only."""
    key = (mapping, c, post)
    if key not in _reference:
        inp, (iw, ih), out, (ow, oh), deg = MAPPINGS[mapping]
        lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, ow, oh)[out]
        rot = cases.rotation(lrp, deg)
        srcs = [oracle.synth_frame(iw, ih, c, 0x7D150000 + 977 * f, 4 if c == 5 else -1) for f in range(N_FRAMES)]
        want = [oracle.reproject(lin, s, lout, ow, oh, 1, 2, rot) for s in srcs]
        if post is not None:
            for w in want:
                oracle.post_process(w, *post)
        for a in srcs + want:
            a.setflags(write=False)
        _reference[key] = (srcs, want)
    return _reference[key]


@pytest.mark.parametrize("c,post", CHANNELS_POST)
@pytest.mark.parametrize("mapping", sorted(MAPPINGS))
def test_tier_dispatch_batches_equal_the_oracle(lrp, torch_cuda, mapping, c, post):
    torch = torch_cuda
    inp, (iw, ih), out, (ow, oh), deg = MAPPINGS[mapping]
    lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, ow, oh)[out]
    rot = cases.rotation(lrp, deg)
    srcs, want = _frames_and_oracle(lrp, mapping, c, post)
    d_srcs = [torch.from_numpy(s.copy()).to("cuda") for s in srcs]
    assert not any(np.array_equal(want[0], w) for w in want[1:])  # (the frames are different frames)
    for knobs in ({"batch_frames": 16}, {}):
        for n in BATCHES:
            with _Knobs(lrp, dict(knobs, geo_cache=1)):
                for _ in range(2):  # the second call finds the geometry-cache entry: the launches under test
                    outs = [torch.full((oh, ow, c), -12345.0, dtype=torch.float32, device="cuda") for _ in range(n)]
                    lrp.reproject_batch([lrp.Image(lin, iw, ih, c, s) for s in d_srcs[:n]],
                                        [lrp.Image(lout, ow, oh, c, d) for d in outs], 1, 2, rot, post=post)
                    torch.cuda.synchronize()
            for f, d in enumerate(outs):
                cases.assert_same_bits(d.cpu().numpy(), want[f], f"{mapping} c={c} post={post} batch of {n} {knobs}: frame {f}")
