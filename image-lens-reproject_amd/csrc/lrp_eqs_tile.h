// lrp_eqs_tile.h — the tile kernel for the equisolid cells (lrp_eqs.h): plain pixels, no frame loop; RGB / RGBA / RGBAZ.
// Included by one unit per sampler (lrp_eqs_tile_{nn,bl,bc}.hip).
#pragma once

#include "lrp_eqs.h"
#include "lrp_kernel_v2.h"

namespace lrp {
template <int Interp, bool OutEqs> struct EqsTilePick {
  static constexpr bool kFrameLoop = false;
  static TileKernelFn get(const KParams &P, int out_idx, int in_mode) {
#define LRP_K3(O, I) reproject_tile_kernel<O, I, Interp, 3, false>
#define LRP_K4(O, I) reproject_tile_kernel<O, I, Interp, 4, false>
#define LRP_K5(O, I) reproject_tile_kernel<O, I, Interp, 5, false>
    static const TileKernelFn t[3][kEqsCells] = {LRP_EQS_CELL_TABLE(LRP_K3), LRP_EQS_CELL_TABLE(LRP_K4), LRP_EQS_CELL_TABLE(LRP_K5)};
#undef LRP_K3
#undef LRP_K4
#undef LRP_K5
    const int cell = eqs_cell_of_index(OutEqs, out_idx, in_mode);
    if (cell < 0 || P.geo_mode == 2 || P.quad != 0 || P.channels < 3 || P.channels > 5) return nullptr;
    return t[P.channels - 3][cell];
  }
};
template <int Interp> hipError_t launch_eqs_tile(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  if (out_lens == kEquisolid) return launch_tile_interp<Interp, EqsTilePick<Interp, true>>(P, eqs_out_index(out_lens), in_mode, stream);
  return launch_tile_interp<Interp, EqsTilePick<Interp, false>>(P, eqs_out_index(out_lens), in_mode, stream);
}
} // namespace lrp
