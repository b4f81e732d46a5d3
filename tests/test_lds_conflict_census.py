"""The bank-conflict model of tools/analysis/lds_conflict_census.py on hand-made address sets (no GPU): a ds_read_b128 is
served in four groups of 16 lanes, the bank of byte address a is (a / 4) mod 64, equal addresses broadcast, every further
distinct address on a busy bank costs one extra cycle — and the lane -> pixel maps it compares."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lds_conflict_census", os.path.join(ROOT, "tools", "analysis", "lds_conflict_census.py"))
census = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(census)


def _wave(group_addrs, group=0):
    """64 byte addresses: `group_addrs` in the lanes of one service group, every other lane on one far-away address."""
    a = np.full(64, 1 << 20, dtype=np.int64)
    a[census.SERVICE_GROUPS[group]] = group_addrs
    return a


def test_service_groups_partition_the_wavefront():
    lanes = np.concatenate(census.SERVICE_GROUPS)
    assert sorted(lanes.tolist()) == list(range(64)) and all(len(g) == 16 for g in census.SERVICE_GROUPS)
    assert census.SERVICE_GROUPS[0].tolist() == [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27]
    assert census.SERVICE_GROUPS[3].tolist() == [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63]


def test_consecutive_slots_are_free():
    for first in (0, 5, 37):
        addrs = 16 * (first + np.arange(16))
        assert census.group_extra_cycles(addrs) == 0
        for g in range(4):
            assert census.read_b128_extra_cycles(_wave(addrs, g)) == 0


def test_stride_of_16_slots_is_16_way():
    addrs = 16 * 16 * np.arange(16)  # every lane on banks 0-3
    assert census.group_extra_cycles(addrs) == 15
    for g in range(4):
        assert census.read_b128_extra_cycles(_wave(addrs, g)) == 15


def test_broadcast_is_free():
    assert census.group_extra_cycles(np.full(16, 4096)) == 0
    assert census.read_b128_extra_cycles(np.full(64, 4096)) == 0
    # two addresses, eight lanes each, 16 slots apart: one extra cycle, not seven
    assert census.group_extra_cycles(np.repeat([0, 256], 8)) == 1


def test_lanes_of_different_groups_do_not_conflict():
    a = np.zeros(64, dtype=np.int64)
    for i, g in enumerate(census.SERVICE_GROUPS):
        a[g] = 256 * i  # four addresses on the same banks, one per group
    assert census.read_b128_extra_cycles(a) == 0


def test_vectorised_form_agrees_with_the_definition():
    rng = np.random.default_rng(7)
    slots = rng.integers(0, 640, size=(200, 64))
    slots[:50] = slots[:50] // 8 * 8  # (many equal addresses and equal banks)
    want = [census.read_b128_extra_cycles(16 * s) for s in slots]
    assert census.extra_cycles_of_slots(slots).tolist() == want


def test_lane_maps():
    for kind in ("row_major", "grouped"):
        row, col = census.lane_map(kind)
        assert sorted(zip(row.tolist(), col.tolist())) == [(r, c) for r in range(4) for c in range(16)]  # a bijection onto the pass
        # quads of consecutive lanes are four consecutive columns of one row: the stores of a quad stay 64 contiguous bytes
        assert (row.reshape(16, 4) == row.reshape(16, 4)[:, :1]).all()
        assert (col.reshape(16, 4) == col.reshape(16, 4)[:, :1] + np.arange(4)).all() and (col[::4] % 4 == 0).all()
    row, _ = census.lane_map("grouped")
    for i, g in enumerate(census.SERVICE_GROUPS):
        assert (row[g] == i).all()  # one output row per service group
    row, _ = census.lane_map("row_major")
    assert sorted(set(row[census.SERVICE_GROUPS[0]].tolist())) == [0, 1]


def test_pitch_rule():
    bw = np.arange(4, 65)
    p = census.pitch_mod16(bw)
    assert (p >= bw).all() and np.isin(p % 16, (0, 1)).all() and (p - bw < 15).all()
    assert census.pitch_mod16(np.array([16, 17, 18, 33]))[[0, 1, 2, 3]].tolist() == [16, 17, 32, 33]
