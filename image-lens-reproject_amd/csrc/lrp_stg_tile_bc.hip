// lrp_stg_tile_bc.hip — bicubic instantiations of the tile kernel (lrp_kernel_v2.h): the stereographic cells.
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_tile_bicubic_stg(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_tile_interp<2, kStgCells>(P, out_lens, in_mode, stream);
}
} // namespace lrp
