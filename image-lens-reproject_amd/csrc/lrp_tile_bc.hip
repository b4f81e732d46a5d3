// lrp_tile_bc.hip — bicubic instantiations of the tile kernel (lrp_kernel_v2.h).
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_tile_bicubic(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  if (launch_cell_set(P, out_lens, in_mode) == kEqsCells) return launch_tile_unit<2, kEqsCells>(P, out_lens, in_mode, stream);
  if (launch_cell_set(P, out_lens, in_mode) == kStgCells) return launch_tile_unit<2, kStgCells>(P, out_lens, in_mode, stream);
  return launch_tile_interp<2>(P, out_lens, in_mode, stream);
}
} // namespace lrp
