// lrp_stg_pixel.hip — instantiations of the reprojection kernel (lrp_kernel_impl.h): the stereographic cells, three samplers.
#include "lrp_kernel_impl.h"

namespace lrp {
hipError_t launch_nearest_stg(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_interp<0, kStgCells>(P, out_lens, in_mode, stream);
}
hipError_t launch_bilinear_stg(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_interp<1, kStgCells>(P, out_lens, in_mode, stream);
}
hipError_t launch_bicubic_stg(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_interp<2, kStgCells>(P, out_lens, in_mode, stream);
}
} // namespace lrp
