"""What one frame of a coefficient-tier block costs a wavefront of the headline kernel in instructions, read from the built object.

reproject_bicubic_win_kernel<kRect, kInEquidistant, 0, 4, Frames, GeoRead, !SS> dispatches on the tier of its one block in
front of the frame loop (lrp_win_kernel.h frame_loop_tier_dispatch, coef_frames): a block of the coefficient tier runs a loop
of its own — the wait, precompute(), four passes, the request of the next frame's window — without a tier test, a rebuilt
flag or a branch over another tier's body, fetches the next frame's pointers where the frame starts and requests the window
rows with 5 scalar instructions per row instead of 9.

tools/isa_kernels.py `frame` counts the instructions of one frame of that loop by class, the request loop for 12 window rows
(the median of the headline's blocks) and precompute() for one trip, planes of the whole block, no tonemap — the path the
headline takes.  The same account of the parent of this change, whose coefficient tier lay inside the generic loop (traced by
leaving out what its forward branches skip, and the tonemap of pass 3 that lay behind its loop's conditional latch): 840 per
frame — packed 380, other VALU 57, LDS 78, vector memory 16, scalar 179, waits 85, branches 45.  With the loop of its own: 710 —
packed 380, other VALU 45, LDS 78, vector memory 16, scalar 108, waits 55, branches 28.

Asserted: the count is at most MAX_PER_FRAME — the count when this was written + 2 %, which absorbs a compiler's reordering —
and that bound lies below the parent's figure.  Skipped when the objects are not built."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj")
HEADLINE = "reproject_bicubic_win_kernelILi0ELi1ELi0ELi4ELb1ELb1ELb0EEE"
PARENT_PER_FRAME = 840
COUNT = 710  # per frame when this was written
MAX_PER_FRAME = COUNT + (COUNT + 49) // 50


def test_headline_coefficient_frame_issues_fewer_instructions_than_before():
    if not os.path.exists(os.path.join(OBJ, "lrp_tile_wing.o")):
        pytest.skip("the kernel objects are not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_kernels
    finally:
        sys.path.pop(0)
    r = isa_kernels.kernel_frame(OBJ, HEADLINE, only=("lrp_tile_wing.o",), rows=12, trips=1, whole=True, post=False)
    assert r is not None, "no loop around four coefficient-tier pass bodies in the headline kernel"
    counts, info = r
    total = sum(counts.values())
    print(f"per frame {total}: " + ", ".join(f"{c} {counts[c]}" for c in isa_kernels.CLASSES) + f" ({info})")
    assert MAX_PER_FRAME < PARENT_PER_FRAME
    assert total <= MAX_PER_FRAME, f"{total} instructions per frame of a coefficient-tier block, at most {MAX_PER_FRAME}: {counts}"
