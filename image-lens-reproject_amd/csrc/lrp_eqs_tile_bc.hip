// lrp_eqs_tile_bc.hip — bicubic instantiations of the tile kernel (lrp_kernel_v2.h): the equisolid cells.
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_tile_bicubic_eqs(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_tile_interp<2, kEqsCells>(P, out_lens, in_mode, stream);
}
} // namespace lrp
