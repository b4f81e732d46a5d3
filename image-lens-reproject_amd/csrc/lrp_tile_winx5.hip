// lrp_tile_winx5.hip — bicubic window-kernel instantiations (lrp_kernel_v2.h): RGBAZ, mirrored columns (pitch rotations).
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_win_bicubic_c5_m3(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_win_bicubic_impl<3, 5>(P, out_lens, in_mode, stream);
}
} // namespace lrp
