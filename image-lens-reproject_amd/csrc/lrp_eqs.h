// lrp_eqs.h — the equisolid fisheye, an opt-in lens extension (include/lrp.h lrp_lens_extensions): its eight (output lens,
// source mode) cells and the pickers that hand the launchers of lrp_kernel_impl.h / lrp_tile_kernel.h / lrp_win_kernel.h
// their kernels.  The instantiations live in units of their own (lrp_eqs_*.hip), so that the code generation of the
// existing units does not move; only plain pixels and blocks are instantiated (no mirror mode, no frame loop).  A launch
// that reads the geometry cache holds no lens math and goes to the existing GeoRead kernels (lrp_capi.cpp).
#pragma once

#include "lrp_params.h"

namespace lrp {

// Cells: equisolid target x the five source modes (0-4), then the rectilinear / equidistant / equirectangular target x the
// equisolid source (5-7); -1: no equisolid lens.  out_lens: kRect / kEquidistant / kEquisolid / kEquirect.
inline int eqs_cell(int out_lens, int in_mode) {
  if (out_lens == kEquisolid) return (in_mode >= 0 && in_mode <= kInEquisolid) ? in_mode : -1;
  if (in_mode != kInEquisolid) return -1;
  return out_lens == kRect ? 5 : out_lens == kEquidistant ? 6 : out_lens == kEquirect ? 7 : -1;
}
constexpr int kEqsCells = 8;
// The launchers of lrp_kernel_impl.h / lrp_tile_kernel.h / lrp_win_kernel.h read out_idx as the target's table index (0
// rectilinear, 1 equidistant, 2 equirectangular) in their shape rules too.  The units of the equisolid cells pass that index —
// the equisolid target as 1, the radial target it is — and tell their pickers by a template argument (OutEqs) whether the
// target is the equisolid lens, so that out_idx means one thing inside the launchers.
inline int eqs_out_index(int out_lens) { return out_lens == kRect ? 0 : out_lens == kEquirect ? 2 : 1; }
inline int eqs_cell_of_index(bool out_eqs, int out_idx, int in_mode) {
  return eqs_cell(out_eqs ? kEquisolid : (out_idx == 0 ? kRect : out_idx == 1 ? kEquidistant : kEquirect), in_mode);
}
// K(out_lens, in_mode): the kernel of one cell, in eqs_cell order.
#define LRP_EQS_CELL_TABLE(K)                                                                                                    \
  {K(kEquisolid, kInRect), K(kEquisolid, kInEquidistant), K(kEquisolid, kInEquirect), K(kEquisolid, kInEquirectLoop),             \
   K(kEquisolid, kInEquisolid), K(kRect, kInEquisolid), K(kEquidistant, kInEquisolid), K(kEquirect, kInEquisolid)}

// Launchers (out_lens / in_mode as eqs_cell takes them).  No geometry-cache reading launch (P.geo_mode 2) goes here.  The
// units that hold the kernels enter them into g_eqs_launchers (defined in lrp_capi.cpp) when the library is loaded, so
// that the host layer links without them (the host-logic drivers under tests/native stub the launchers they know); a
// missing entry is an error, never a fall-back.
using EqsLaunchFn = hipError_t (*)(const KParams &P, int out_lens, int in_mode, hipStream_t stream);
struct EqsLaunchers {
  hipError_t (*pixel)(const KParams &P, int interpolation, int out_lens, int in_mode, hipStream_t stream); // lrp_eqs_pixel.hip
  EqsLaunchFn tile[3]; // nearest, bilinear, bicubic: lrp_eqs_tile_{nn,bl,bc}.hip
  EqsLaunchFn win;     // lrp_eqs_win.hip
};
extern EqsLaunchers g_eqs_launchers;

} // namespace lrp
