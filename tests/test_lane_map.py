"""CPU: the lane -> pixel maps of a 16 x 4 pass of the window kernel (csrc/lrp_lane_map.h: row-major, rows, patches), printed by
tests/native/lane_map_driver.cpp — plain g++, the header includes no HIP header, and its static_asserts hold when the driver
builds — against the Python tables of tools/analysis/lds_conflict_census.py, and the properties the kernel counts on, against
the LDS's service groups of a ds_read_b128: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and both + 32.

... and the census's conflict model on the slots the patches map is about: the 3 x 3 source texels under a 4 x 4 patch of a
2x-magnified mapping lie on distinct banks at pitch 13, the 16 pixels of an output row that steps to the next window row do
not."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-lens-reproject_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "native", "_build")
_spec = importlib.util.spec_from_file_location("lds_conflict_census", os.path.join(ROOT, "tools", "analysis", "lds_conflict_census.py"))
census = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(census)

MAPS = ("row_major", "rows", "patches")
_G0 = list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28))
_G1 = list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))
GROUPS = [_G0, _G1, [l + 32 for l in _G0], [l + 32 for l in _G1]]  # (written out here: not taken from the code under test)


@pytest.fixture(scope="module")
def header_maps():
    """name -> (group[64], row[64], col[64]) as the header computes them."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "lane_map_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "native", "lane_map_driver.cpp"), "-o", exe],
                   check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    maps = {m: np.full((3, 64), -1, dtype=np.int64) for m in MAPS}
    for line in r.stdout.split("\n"):
        if line:
            name, lane, group, row, col = line.split()
            maps[name][:, int(lane)] = (int(group), int(row), int(col))
    assert all((m >= 0).all() for m in maps.values())
    return maps


@pytest.mark.parametrize("name", MAPS)
def test_header_and_census_agree(header_maps, name):
    row, col = census.lane_map(name)
    assert header_maps[name][1].tolist() == row.tolist() and header_maps[name][2].tolist() == col.tolist()
    for g, lanes in enumerate(GROUPS):
        assert (header_maps[name][0][lanes] == g).all()  # lane_service_group is the hardware's grouping
        assert census.SERVICE_GROUPS[g].tolist() == lanes


def test_grouped_is_the_rows_map():
    assert [a.tolist() for a in census.lane_map("grouped")] == [a.tolist() for a in census.lane_map("rows")]


@pytest.mark.parametrize("name", MAPS)
def test_bijection_quads_and_stores(header_maps, name):
    _, row, col = header_maps[name]
    # a bijection onto the 16 x 4 pass: the wavefront stores every pixel of the pass once, 4 rows x 256 B of RGBA
    assert sorted(zip(row.tolist(), col.tolist())) == [(r, c) for r in range(4) for c in range(16)]
    # every aligned quad of lanes is four consecutive columns of one row, in lane order: 64 contiguous bytes
    assert (row.reshape(16, 4) == row.reshape(16, 4)[:, :1]).all()
    assert (col.reshape(16, 4) == col.reshape(16, 4)[:, :1] + np.arange(4)).all() and (col[::4] % 4 == 0).all()


def test_patches_map(header_maps):
    _, row, col = header_maps["patches"]
    for g, lanes in enumerate(GROUPS):
        # each service group is one 4 x 4 patch: rows 0-3 x patch columns 4g .. 4g + 3, every pixel of it once
        assert sorted(zip(row[lanes].tolist(), col[lanes].tolist())) == [(r, 4 * g + c) for r in range(4) for c in range(4)]
    # every aligned group of eight lanes is one whole 128-byte line of the output: eight RGBA pixels from a multiple of eight
    for l0 in range(0, 64, 8):
        assert len(set(row[l0:l0 + 8].tolist())) == 1
        cols = sorted(col[l0:l0 + 8].tolist())
        assert cols == list(range(cols[0], cols[0] + 8)) and cols[0] % 8 == 0
    # the formulas of the map, lane by lane
    for lane in range(64):
        q = (lane >> 2) & 7
        par = bin(q).count("1") & 1
        assert (row[lane], col[lane]) == (q >> 1, 4 * (2 * (lane >> 5) + par) + (lane & 3))


def test_rows_and_row_major_groups(header_maps):
    _, row, col = header_maps["rows"]
    for g, lanes in enumerate(GROUPS):
        assert (row[lanes] == g).all() and sorted(col[lanes].tolist()) == list(range(16))  # one output row per service group
    _, row, _ = header_maps["row_major"]
    assert sorted(set(row[GROUPS[0]].tolist())) == [0, 1]  # half of two rows
    assert (header_maps["row_major"][1] == np.arange(64) // 16).all() and (header_maps["row_major"][2] == np.arange(64) % 16).all()


def test_8x2_patches_of_the_census():
    row, col = census.lane_map("patches_8x2")
    assert sorted(zip(row.tolist(), col.tolist())) == [(r, c) for r in range(4) for c in range(16)]
    for g, lanes in enumerate(GROUPS):
        want = [(2 * (g >> 1) + r, 8 * (g & 1) + c) for r in range(2) for c in range(8)]
        assert sorted(zip(row[lanes].tolist(), col[lanes].tolist())) == want


# ---- the conflict model on hand-made slots --------------------------------------------------------------------------
PITCH = 13


def _pass_slots(name, texel_of_pixel):
    """[1, 64] window slots of a pass's first read under map `name`; texel_of_pixel(row, col) -> (window row, window column)."""
    row, col = census.lane_map(name)
    slots = [wy * PITCH + wx for wy, wx in (texel_of_pixel(int(r), int(c)) for r, c in zip(row, col))]
    return np.array([slots], dtype=np.int64)


def test_3x3_texels_of_a_patch_are_free_at_pitch_13():
    # the nine slots of a 3 x 3 texel patch, every lane of a service group on one of them (all nine used)
    nine = [wy * PITCH + wx for wy in range(3) for wx in range(3)]
    assert len({s % 16 for s in nine}) == 9  # distinct banks: 0 1 2, 13 14 15, 10 11 12
    addrs = 16 * np.array((nine * 2)[:16])
    assert census.group_extra_cycles(addrs) == 0
    for first in range(0, 40):  # ... wherever the patch lies in the window
        assert census.group_extra_cycles(addrs + 16 * first) == 0
    # a 2x-magnified pass under the patches map: pixel (r, c) reads texel (r / 2, c / 2), phases chosen so that every 4 x 4
    # patch spans three texel rows and three texel columns
    slots = _pass_slots("patches", lambda r, c: ((r + 1) // 2, (c + 1) // 2))
    for j in range(4):  # the four consecutive slots of a read sequence move every lane alike
        assert census.extra_cycles_of_slots(slots + j).tolist() == [0]
    assert census.read_b128_extra_cycles(16 * slots[0]) == 0


def test_a_row_that_steps_a_window_row_conflicts():
    # 16 pixels of one output row, 2x magnified (eight texel columns 2-9) and slightly rotated: from pixel 8 on they read the
    # next window row — slots 2-5 and 13 + 6 .. 13 + 9 = 19-22: 19, 20, 21 lie on the banks of 3, 4, 5
    def texel(c):
        return (1 if c >= 8 else 0), 2 + c // 2

    addrs = 16 * np.array([wy * PITCH + wx for wy, wx in map(texel, range(16))])
    assert census.group_extra_cycles(addrs) >= 1
    # as a pass: under the rows map each of the four service groups is such a row (two addresses on a bank: one extra cycle
    # each); under the patches map a group reads two texel columns in three window rows, six slots on distinct banks
    for name, want in (("rows", 4), ("patches", 0)):
        extra = int(census.extra_cycles_of_slots(_pass_slots(name, lambda r, c: (texel(c)[0] + (r + 1) // 2, texel(c)[1])))[0])
        assert extra == want, (name, extra)
