// lrp_cells.h — from (out_lens, in_mode) to a kernel.  A launch is described by the output lens and the source mode in the
// ids of lrp_params.h, from lrp_capi.cpp down to here; a kernel variant (the pixel kernel, the tile kernel with the frame
// loop, the window kernel of a mirror mode ...) states its cells as a functor
//     struct Cell { template <int OutLens, int InMode> static constexpr KernelFn kernel(); };
// that returns the instantiation of the cell, or nullptr for a cell the variant does not hold; cell_kernel<Cell>() is the
// table of all of them.  Which cells a variant holds is said once, by the predicates below.
#pragma once

#include <array>
#include <utility>

#include "lrp_params.h"

namespace lrp {

using KernelFn = void (*)(const KParams);

constexpr bool has_equisolid(int out_lens, int in_mode) { return out_lens == kEquisolid || in_mode == kInEquisolid; }
constexpr bool has_stereographic(int out_lens, int in_mode) { return out_lens == kStereographic || in_mode == kInStereographic; }
// A cell with a lens of the opt-in extensions (lrp_lens_extensions) on either side: plain pixels and blocks only.
constexpr bool has_extension_lens(int out_lens, int in_mode) { return has_equisolid(out_lens, in_mode) || has_stereographic(out_lens, in_mode); }

// ---- which cells a variant holds ------------------------------------------------------------------
// Mirror modes (lrp_win_kernel.h QMode; the tile kernel's P.quad): rows-only needs the column-separable source x — no
// equidistant lens on either side —, columns-only a rectilinear target, shared rays the equidistant target; the extension
// lenses (equisolid, stereographic) have none.
constexpr bool mirror_cell(int qmode, int out_lens, int in_mode) {
  return qmode == 0 || (!has_extension_lens(out_lens, in_mode) && (qmode != 2 || (out_lens != kEquidistant && in_mode != kInEquidistant)) &&
                        (qmode != 3 || out_lens == kRect) && (qmode != 4 || out_lens == kEquidistant));
}
// The frame loop of the batched launches: not for the extension lenses (a batch renders a frame per workgroup row, blockIdx.y).
constexpr bool frame_loop_cell(int out_lens, int in_mode) { return !has_extension_lens(out_lens, in_mode); }
// GeoRead kernels hold no lens math: one per source mode, the output lens kRect by convention — and the clamped,
// non-wrapping equidistant source's serves the equisolid and the stereographic source (geo_read_in_mode).
constexpr bool geo_read_cell(int out_lens, int in_mode) { return out_lens == kRect && in_mode != kInEquisolid && in_mode != kInStereographic; }
constexpr int geo_read_in_mode(int in_mode) { return (in_mode == kInEquisolid || in_mode == kInStereographic) ? kInEquidistant : in_mode; }
// ... and the window kernel's big-window variants, "kEquirect" by convention (lrp_win_kernel.h kBigWin).
constexpr bool geo_big_cell(int out_lens, int in_mode) {
  return out_lens == kEquirect && (in_mode == kInRect || in_mode == kInEquirect || in_mode == kInEquirectLoop);
}

// ---- which unit compiles a cell -------------------------------------------------------------------
// The cells with an extension lens are instantiated by units of their own, next to the units of the reference's lenses: a
// unit's launcher takes its set as a template argument and its tables are null elsewhere.  kStgCells (lrp_stg_*.o): every
// cell with a stereographic lens, the two it shares with the equisolid lens included; kEqsCells (lrp_eqs_*.o): the other
// cells with an equisolid lens.  Those objects are lines of units.list: lrp_{pixel,tile,win}_unit.hip with the set as a define.
enum CellSet : int { kStdCells = 0, kEqsCells = 1, kStgCells = 2 };
constexpr CellSet cell_set_of(int out_lens, int in_mode) {
  return has_stereographic(out_lens, in_mode) ? kStgCells : has_equisolid(out_lens, in_mode) ? kEqsCells : kStdCells;
}
constexpr bool in_cell_set(CellSet set, int out_lens, int in_mode) { return cell_set_of(out_lens, in_mode) == set; }
// The set whose units hold the kernel of a launch (a launch that reads the geometry cache: a GeoRead kernel, see above).
inline CellSet launch_cell_set(const KParams &P, int out_lens, int in_mode) {
  return P.geo_mode != 2 ? cell_set_of(out_lens, in_mode) : kStdCells;
}

// ---- the table ------------------------------------------------------------------------------------
// Rows by lens id, columns by source mode.  An id that names no lens would be a row of null entries (today every id
// 0 .. kLensIds - 1 names one).
constexpr int kLensIds = 5, kInModes = 6;
constexpr bool is_lens_id(int id) { return id == kRect || id == kEquidistant || id == kEquisolid || id == kStereographic || id == kEquirect; }
static_assert(kInRect == 0 && kInEquidistant == 1 && kInEquirect == 2 && kInEquirectLoop == 3 && kInEquisolid == 4 && kInStereographic == kInModes - 1, "source modes: 0 .. kInModes - 1");
static_assert(kEquirect == kLensIds - 1 && kStereographic < kLensIds, "lens ids: 0 .. kLensIds - 1");

template <class Cell, int OutLens, int InMode> constexpr KernelFn cell_entry() {
  if constexpr (is_lens_id(OutLens))
    return Cell::template kernel<OutLens, InMode>();
  else
    return nullptr;
}
template <class Cell, int OutLens, int... InMode>
constexpr std::array<KernelFn, kInModes> cell_row(std::integer_sequence<int, InMode...>) {
  return {{cell_entry<Cell, OutLens, InMode>()...}};
}
template <class Cell, int... OutLens>
constexpr std::array<std::array<KernelFn, kInModes>, kLensIds> cell_table(std::integer_sequence<int, OutLens...>) {
  return {{cell_row<Cell, OutLens>(std::make_integer_sequence<int, kInModes>{})...}};
}
// The kernel of cell (out_lens, in_mode) of a variant; nullptr: the variant does not hold it.
template <class Cell> KernelFn cell_kernel(int out_lens, int in_mode) {
  static const std::array<std::array<KernelFn, kInModes>, kLensIds> table = cell_table<Cell>(std::make_integer_sequence<int, kLensIds>{});
  if (out_lens < 0 || out_lens >= kLensIds || in_mode < 0 || in_mode >= kInModes) return nullptr;
  return table[out_lens][in_mode];
}

} // namespace lrp
