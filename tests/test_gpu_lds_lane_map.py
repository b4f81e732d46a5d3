"""-m gpu: a one-block frame-loop window kernel may map lanes to pixels so that each LDS service group of a ds_read_b128
renders one output row of a pass (lrp_win_plan.h win_lane_pixel<true>; lrp_win_kernel.h frame_loop_grouped_lanes says which
do: the RGBA kernel of the equidistant source) instead of row-major.  Everything a lane holds of a pass — weights, window
address, store offset, its slot in the RGBAZ exchange, its share of a corner block's stores — follows from (row, column) of
its pixel, so under either map the rendered words must be the oracle's, bit for bit: every source mode and channel count
is rendered, whichever map its kernel takes.

Batches of 1, 2 and 16 frames through reproject_batch, rendered twice so that the second call reads the geometry cache:
with batch_frames 16 the batches of 2 and 16 take the frame-loop kernels (2: a frame loop that ends at once; a batch of 1 is
a single launch of the kernels without the frame loop — the row-major map — and must give the same words), and under the
launcher's own choice of frames per wavefront as well.  RGB, RGBA and RGBAZ.  The output is 40 x 36: three block columns
and three block rows, the last of each partial (8 columns, 4 rows: lanes and whole passes beyond the image store the
clamped pixel again).  The mappings are those of tests/test_gpu_frame_loop_pass_state.py — every tier of these kernels:
coefficient planes, raw taps, gathers, edge row / edge column / corner blocks — with sources of about 64 x 64.  Blocks per
tier of the nine blocks of each (the plan of tools/analysis/lds_conflict_census.py on the oracle's coordinates):
  eqd_rect_magnified   coefficient 6, raw 3              eqr_rect_magnified    coefficient 3, raw 1, gathers 5
  eqr_loop_rect        coefficient 6, gathers 3          rect_rect_1to1        coefficient 2, raw 3, gathers 4
  eqd_eqd_minified     gathers 9                         tele_in_wide(_rolled) gathers 8, corner 1
(At 40 x 36 the tele source covers 14 x 13 output pixels in the middle block: no block lies beyond one side of it only, so
the edge tiers have no block here; tests/test_gpu_frame_loop_pass_state.py renders them at 200 x 136.)"""
import numpy as np
import pytest

import cases
import oracle_binding as oracle

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True

OUT_W, OUT_H = 40, 36
# name -> (input lens, input size, output lens, rotation in degrees)
MAPPINGS = {
    "eqd_rect_magnified": ("eqd180", (56, 56), "rect", (30.0, -15.0, 5.0)),
    "eqr_rect_magnified": ("eqr_part", (64, 32), "rect", (30.0, -15.0, 5.0)),
    "eqr_loop_rect": ("eqr_full", (80, 40), "rect", (180.0, 0.0, 0.0)),
    "rect_rect_1to1": ("rect", (52, 56), "rect", (2.0, -1.0, 3.0)),
    "eqd_eqd_minified": ("eqd180", (128, 128), "eqd180", (10.0, 5.0, 0.0)),
    "tele_in_wide": ("rect_tele", (64, 56), "rect", None),
    "tele_in_wide_rolled": ("rect_tele", (64, 56), "rect", (0.0, 0.0, 1.0)),
}
CHANNELS = (3, 4, 5)
BATCHES = (1, 2, 16)
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


def _frames_and_oracle(lrp, mapping, c):
    """The 16 source frames of (mapping, c) and the oracle's rendering of each: computed once, shared, read-only."""
    key = (mapping, c)
    if key not in _reference:
        inp, (iw, ih), out, deg = MAPPINGS[mapping]
        lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, OUT_W, OUT_H)[out]
        rot = cases.rotation(lrp, deg)
        srcs = [oracle.synth_frame(iw, ih, c, 0x1A9E0000 + 977 * f, 4 if c == 5 else -1) for f in range(N_FRAMES)]
        want = [oracle.reproject(lin, s, lout, OUT_W, OUT_H, 1, 2, rot) for s in srcs]
        for a in srcs + want:
            a.setflags(write=False)
        _reference[key] = (srcs, want)
    return _reference[key]


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("mapping", sorted(MAPPINGS))
def test_frame_loop_batches_equal_the_oracle(lrp, torch_cuda, mapping, c):
    torch = torch_cuda
    inp, (iw, ih), out, deg = MAPPINGS[mapping]
    lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, OUT_W, OUT_H)[out]
    rot = cases.rotation(lrp, deg)
    srcs, want = _frames_and_oracle(lrp, mapping, c)
    d_srcs = [torch.from_numpy(s.copy()).to("cuda") for s in srcs]
    assert not any(np.array_equal(want[0], w) for w in want[1:])  # (the frames are different frames)
    for knobs in ({"batch_frames": 16}, {}):
        for n in BATCHES:
            with _Knobs(lrp, dict(knobs, geo_cache=1)):
                for _ in range(2):  # the second call finds the geometry-cache entry: the launches under test
                    outs = [torch.full((OUT_H, OUT_W, c), -12345.0, dtype=torch.float32, device="cuda") for _ in range(n)]
                    lrp.reproject_batch([lrp.Image(lin, iw, ih, c, s) for s in d_srcs[:n]],
                                        [lrp.Image(lout, OUT_W, OUT_H, c, d) for d in outs], 1, 2, rot)
                    torch.cuda.synchronize()
            for f, d in enumerate(outs):
                cases.assert_same_bits(d.cpu().numpy(), want[f], f"{mapping} c={c} batch of {n} {knobs}: frame {f}")
