// lrp_lane_map.h — which lane of a wavefront renders which pixel of a 16 x 4 pass of the window kernel (lrp_win_plan.h
// win_lane_pixel, lrp_win_kernel.h frame_loop_lane_map).  Plain constexpr C++, no HIP header: tests/native/lane_map_driver.cpp
// includes it on the host.
//
// The LDS serves a ds_read_b128 in four groups of 16 lanes — {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32
// (MI355X_MICROARCH.md, LDS) — and only lanes of one group can conflict.  With q = bits 2-4 of the lane (its quad within the
// half wavefront) the group of a lane is 2 * (lane >> 5) + parity(q).
//   row-major  lane = 16 row + column: half of two different output rows in every group.
//   rows       each group renders ONE output row of the pass; the quad's place in the row is q >> 1.
//   patches    each group renders ONE 4 x 4 patch: patch columns 4 group .. 4 group + 3, the quad's row is q >> 1.
// Under every map an aligned quad of lanes is four consecutive columns of one row (a quad stores 64 contiguous bytes of RGBA)
// and the wavefront stores the same 4 x 256 B per pass; under row-major and patches an aligned group of eight lanes covers eight
// consecutive columns of one row (one whole 128-byte line; under rows it is the same half line of two rows).
#pragma once

namespace lrp {

enum WinLaneMap : int { kLaneRowMajor = 0, kLaneRows = 1, kLanePatches = 2 };

constexpr int kLanePassCols = 16, kLanePassRows = 4;

constexpr int lane_quad_parity(int lane) { return __builtin_popcount((unsigned)lane & 28u) & 1; }
// the LDS service group of a lane's ds_read_b128
constexpr int lane_service_group(int lane) { return ((lane >> 5) << 1) | lane_quad_parity(lane); }

constexpr int lane_pixel_row(WinLaneMap map, int lane) {
  return map == kLaneRows ? lane_service_group(lane) : map == kLanePatches ? (lane >> 3) & 3 : lane / kLanePassCols;
}
constexpr int lane_pixel_col(WinLaneMap map, int lane) {
  return map == kLaneRows      ? ((lane >> 1) & 12) | (lane & 3)
         : map == kLanePatches ? (lane_service_group(lane) << 2) | (lane & 3)
                               : lane & (kLanePassCols - 1);
}

namespace lane_map_checks {
// a bijection onto the 16 x 4 pass: every pixel is some lane's
constexpr bool bijection(WinLaneMap m) {
  unsigned long long seen = 0;
  for (int l = 0; l < 64; ++l) {
    const int r = lane_pixel_row(m, l), c = lane_pixel_col(m, l);
    if (r < 0 || r >= kLanePassRows || c < 0 || c >= kLanePassCols) return false;
    seen |= 1ull << (r * kLanePassCols + c);
  }
  return seen == ~0ull;
}
// every aligned quad of lanes is four consecutive columns of one row in lane order, the first of them a multiple of four
constexpr bool aligned_quads(WinLaneMap m) {
  for (int l = 0; l < 64; ++l) {
    const int l0 = l & ~3;
    if (lane_pixel_row(m, l) != lane_pixel_row(m, l0) || lane_pixel_col(m, l) != lane_pixel_col(m, l0) + (l - l0)) return false;
    if (lane_pixel_col(m, l0) % 4 != 0) return false;
  }
  return true;
}
// every aligned group of eight lanes covers columns 0-7 or 8-15 of one row (its two quads in either order)
constexpr bool aligned_lines(WinLaneMap m) {
  for (int l0 = 0; l0 < 64; l0 += 8) {
    unsigned cols = 0;
    for (int l = l0; l < l0 + 8; ++l) {
      if (lane_pixel_row(m, l) != lane_pixel_row(m, l0)) return false;
      cols |= 1u << lane_pixel_col(m, l);
    }
    if (cols != 0x00ffu && cols != 0xff00u) return false;
  }
  return true;
}
// the service groups are {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and both + 32
constexpr bool service_groups() {
  for (int l = 0; l < 64; ++l) {
    const int h = l & 31;
    const int g = ((h < 4) || (h >= 12 && h < 16) || (h >= 20 && h < 28)) ? 0 : 1;
    if (lane_service_group(l) != 2 * (l >> 5) + g) return false;
  }
  return true;
}
// the box of the pixels of service group g: rows x columns, -1 where its 16 lanes do not fill that box
constexpr int group_box(WinLaneMap m, int g, bool want_rows) {
  int r0 = 99, r1 = -1, c0 = 99, c1 = -1, n = 0;
  for (int l = 0; l < 64; ++l) {
    if (lane_service_group(l) != g) continue;
    const int r = lane_pixel_row(m, l), c = lane_pixel_col(m, l);
    r0 = r < r0 ? r : r0;
    r1 = r > r1 ? r : r1;
    c0 = c < c0 ? c : c0;
    c1 = c > c1 ? c : c1;
    ++n;
  }
  const int rows = r1 - r0 + 1, cols = c1 - c0 + 1;
  if (n != 16 || rows * cols != 16) return -1; // (with the bijection: 16 distinct pixels in a box of 16)
  return want_rows ? rows : cols;
}
constexpr bool group_boxes(WinLaneMap m, int rows, int cols) {
  for (int g = 0; g < 4; ++g)
    if (group_box(m, g, true) != rows || group_box(m, g, false) != cols) return false;
  return true;
}
static_assert(service_groups(), "lane_service_group is the LDS's grouping of a ds_read_b128");
static_assert(bijection(kLaneRowMajor) && bijection(kLaneRows) && bijection(kLanePatches), "every map is a bijection onto the pass");
static_assert(aligned_quads(kLaneRowMajor) && aligned_quads(kLaneRows) && aligned_quads(kLanePatches),
              "an aligned quad of lanes is four consecutive columns of one row");
static_assert(aligned_lines(kLaneRowMajor) && aligned_lines(kLanePatches) && !aligned_lines(kLaneRows),
              "row-major, patches: an aligned group of eight lanes is one whole 128-byte line of an RGBA output row (rows: two half lines)");
static_assert(group_boxes(kLaneRows, 1, 16), "rows: a service group is one output row of the pass");
static_assert(group_boxes(kLanePatches, 4, 4), "patches: a service group is one 4 x 4 patch");
static_assert(group_box(kLaneRowMajor, 0, true) == -1, "row-major: a service group is half of two rows, no box");
} // namespace lane_map_checks

} // namespace lrp
