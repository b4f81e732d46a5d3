"""-m gpu: the patches lane map of the one-block frame-loop window kernels (csrc/lrp_lane_map.h kLanePatches: each LDS service
group of a ds_read_b128 renders one 4 x 4 patch of a 16 x 4 pass; lrp_win_kernel.h frame_loop_lane_map says which kernels
take it) against the oracle, bit for bit, on the magnified mappings the map is for.  Everything a lane holds of a pass —
weights, window address, store offset, its slot in the RGBAZ exchange — follows from (row, column) of its pixel, so the
rendered words must be the oracle's whichever map a kernel takes: RGB, RGBA and RGBAZ of the fisheye source and of both
panorama sources are rendered, adopters and the others alike (the rectilinear source, which keeps row-major, is
tests/test_gpu_lds_lane_map.py's).

Mappings, all into a 40 x 36 rectilinear view (three block columns and three block rows, the last of each partial: 8 columns,
4 rows — lanes and whole passes beyond the image store the clamped pixel again):
  eqd_2x        the headline's geometry, unrotated: equidistant fisheye of fov pi, 40 x 40, magnified about 2x
  eqr_loop_4x   a full panorama of 40 x 20, magnified 4x (a 4 x 4 patch reads two texel rows and columns)
  eqr_part_4x   a partial panorama of 16 x 8, magnified about 4x
Batches of 2, 3 and 16 frames through reproject_batch, each rendered twice so that the second call reads the geometry cache
(the launches under test: the frame-loop kernels), with batch_frames 16 and under the launcher's own choice of frames per
wavefront."""
import numpy as np
import pytest

import cases
import oracle_binding as oracle

pytestmark = pytest.mark.gpu
USES_GEO_CACHE = True

OUT_W, OUT_H = 40, 36
# name -> (input lens, input size, rotation in degrees)
MAPPINGS = {
    "eqd_2x": ("eqd180", (40, 40), None),
    "eqr_loop_4x": ("eqr_full", (40, 20), None),
    "eqr_part_4x": ("eqr_part", (16, 8), None),
}
CHANNELS = (3, 4, 5)
BATCHES = (2, 3, 16)
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
        inp, (iw, ih), deg = MAPPINGS[mapping]
        lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, OUT_W, OUT_H)["rect"]
        srcs = [oracle.synth_frame(iw, ih, c, 0x1B7C0000 + 977 * f, 4 if c == 5 else -1) for f in range(N_FRAMES)]
        want = [oracle.reproject(lin, s, lout, OUT_W, OUT_H, 1, 2, cases.rotation(lrp, deg)) for s in srcs]
        for a in srcs + want:
            a.setflags(write=False)
        _reference[key] = (srcs, want)
    return _reference[key]


@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("mapping", sorted(MAPPINGS))
def test_magnified_frame_loop_batches_equal_the_oracle(lrp, torch_cuda, mapping, c):
    torch = torch_cuda
    inp, (iw, ih), deg = MAPPINGS[mapping]
    lin, lout = cases.lenses(lrp, iw, ih)[inp], cases.lenses(lrp, OUT_W, OUT_H)["rect"]
    rot = cases.rotation(lrp, deg)
    srcs, want = _frames_and_oracle(lrp, mapping, c)
    d_srcs = [torch.from_numpy(s.copy()).to("cuda") for s in srcs]
    assert not any(np.array_equal(want[0], w) for w in want[1:])  # (the frames are different frames)
    for knobs in ({"batch_frames": 16}, {}):
        for n in BATCHES:
            with _Knobs(lrp, dict(knobs, geo_cache=1)):
                for call in range(2):  # the second call finds the geometry-cache entry: the launches under test
                    outs = [torch.full((OUT_H, OUT_W, c), -12345.0, dtype=torch.float32, device="cuda") for _ in range(n)]
                    lrp.reproject_batch([lrp.Image(lin, iw, ih, c, s) for s in d_srcs[:n]],
                                        [lrp.Image(lout, OUT_W, OUT_H, c, d) for d in outs], 1, 2, rot)
                    torch.cuda.synchronize()
                    for f, d in enumerate(outs):
                        cases.assert_same_bits(d.cpu().numpy(), want[f], f"{mapping} c={c} batch of {n} {knobs} call {call}: frame {f}")
