// lrp_tile_win3.hip — bicubic window-kernel instantiations (lrp_kernel_v2.h): RGB, plain blocks.
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_win_bicubic_c3_m0(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_win_bicubic_impl<0, 3>(P, out_lens, in_mode, stream);
}
} // namespace lrp
