// lrp_eqs_win.h — the LDS-window bicubic kernel for the equisolid cells (lrp_eqs.h): plain blocks, no frame loop, the
// geometry-cache side output (kGeoWrite) of the single launches; SS: the supersampling instantiations (num_samples 2-4).
// Included by one unit per (channel count, SS) (lrp_eqs_win{3,4,5}.hip, lrp_eqs_wins{3,4,5}.hip).
#pragma once

#include "lrp_eqs.h"
#include "lrp_kernel_v2.h"

namespace lrp {
template <int CH, bool SS, bool OutEqs> struct EqsWinPick {
  static constexpr bool kFrameLoop = false;
  static TileKernelFn get(const KParams &P, int out_idx, int in_mode) {
#define LRP_KW(O, I) reproject_bicubic_win_kernel<O, I, 0, CH, false, false, SS>
    static const TileKernelFn t[kEqsCells] = LRP_EQS_CELL_TABLE(LRP_KW);
#undef LRP_KW
    const int cell = eqs_cell_of_index(OutEqs, out_idx, in_mode);
    if (cell < 0 || P.geo_mode == 2 || P.win_mode != 0) return nullptr;
    return t[cell];
  }
};
template <int CH, bool SS> hipError_t launch_eqs_win_impl(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  if (out_lens == kEquisolid) return launch_win_bicubic_impl<0, CH, false, SS, EqsWinPick<CH, SS, true>>(P, eqs_out_index(out_lens), in_mode, stream);
  return launch_win_bicubic_impl<0, CH, false, SS, EqsWinPick<CH, SS, false>>(P, eqs_out_index(out_lens), in_mode, stream);
}
} // namespace lrp
