"""What a coefficient-tier pass of the headline kernel issues beside its arithmetic, read from the built object.

reproject_bicubic_win_kernel<kRect, kInEquidistant, 0, 4, Frames, GeoRead, !SS> holds a pass's lane state across the frames of
its block (lrp_win_kernel.h PassLane, hoist level 2): a pass derives three plane addresses from the held window address and
hfx, hfy from the held weights, about 5 vector instructions, where it used to truncate, convert, subtract, multiply, clamp
and rebuild a 64-bit store address.

tools/isa_kernels.py `passes` finds the pass bodies by their group of 16 ds_read_b128 and tells the tiers apart by their
packed arithmetic (coefficient tier: 82 v_pk_* for the cubics + 2 for 0.0f + s; raw taps: 170).  It counts the non-packed VALU
instructions of a tier's own stretch and of the store's basic block; the blocks of flag tests between the two are left out,
so its counts are lower than a count of everything between two stores (by hand, on the parent of this change: about 33 per
coefficient-tier pass).  With the same tool: coefficient-tier bodies 30 / 23 / 25 / 24 on the parent, 10 / 6 / 6 / 10 with the
held state (the first body carries the re-materialised tier flags, the last one the request of the next frame's window);
raw-tap bodies 18-24 on the parent, 6-7 now.

Asserted: exactly four coefficient-tier bodies — a block has four passes —, each with 16 ds_read_b128, at least 82 v_pk_* and at
most 10 non-packed VALU instructions up to its global_store_dwordx4.  Skipped when the objects are not built."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj")
HEADLINE = "reproject_bicubic_win_kernelILi0ELi1ELi0ELi4ELb1ELb1ELb0EEE"
MAX_VALU_PER_PASS = 10


def test_headline_pass_bodies_issue_few_unpacked_valu():
    if not os.path.exists(os.path.join(OBJ, "lrp_tile_wing.o")):
        pytest.skip("the kernel objects are not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_kernels
    finally:
        sys.path.pop(0)
    bodies = isa_kernels.kernel_passes(OBJ, HEADLINE, only=("lrp_tile_wing.o",))
    assert bodies is not None, "the headline kernel is not in lrp_tile_wing.o"
    for k, b in enumerate(bodies):
        print(f"pass body {k} ({b['tier']}): ds_read_b128 {b['ds_read_b128']} packed {b['packed']} non-packed VALU {b['valu']}: {b['valu_text']}")
    coef = [b for b in bodies if b["tier"] == "coef"]
    assert len(coef) == 4, f"{len(coef)} coefficient-tier pass bodies found, a block has four passes"
    for k, b in enumerate(coef):
        assert b["ds_read_b128"] == 16 and 82 <= b["packed"] < 120, (k, b)
        assert b["valu"] <= MAX_VALU_PER_PASS, f"coefficient-tier pass {k}: {b['valu']} non-packed VALU instructions: {b['valu_text']}"
