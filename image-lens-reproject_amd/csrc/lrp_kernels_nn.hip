// lrp_kernels_nn.hip — nearest instantiations of the reprojection kernel
// (one translation unit per interpolation mode; see lrp_kernel_impl.h).
#include "lrp_kernel_impl.h"

namespace lrp {
hipError_t launch_nearest(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  if (launch_cell_set(P, out_lens, in_mode) == kEqsCells) return launch_pixel_unit<0, kEqsCells>(P, out_lens, in_mode, stream);
  if (launch_cell_set(P, out_lens, in_mode) == kStgCells) return launch_pixel_unit<0, kStgCells>(P, out_lens, in_mode, stream);
  return launch_interp<0>(P, out_lens, in_mode, stream);
}
} // namespace lrp
