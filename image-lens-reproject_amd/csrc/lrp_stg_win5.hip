// lrp_stg_win5.hip — bicubic window-kernel instantiations (lrp_kernel_v2.h): RGBAZ, plain blocks, the stereographic cells.
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_win_bicubic_c5_m0_stg(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_win_bicubic_impl<0, 5, false, false, kStgCells>(P, out_lens, in_mode, stream);
}
} // namespace lrp
