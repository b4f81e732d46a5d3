// lrp_eqs_pixel.hip — instantiations of the reprojection kernel (lrp_kernel_impl.h): the equisolid cells, three samplers.
#include "lrp_kernel_impl.h"

namespace lrp {
hipError_t launch_nearest_eqs(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_interp<0, kEqsCells>(P, out_lens, in_mode, stream);
}
hipError_t launch_bilinear_eqs(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_interp<1, kEqsCells>(P, out_lens, in_mode, stream);
}
hipError_t launch_bicubic_eqs(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_interp<2, kEqsCells>(P, out_lens, in_mode, stream);
}
} // namespace lrp
