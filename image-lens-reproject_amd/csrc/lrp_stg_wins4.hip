// lrp_stg_wins4.hip — bicubic window-kernel instantiations (lrp_kernel_v2.h): RGBA, num_samples 2-4 (the SS instantiations), the stereographic cells.
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_win_bicubic_ss_c4_stg(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_win_bicubic_impl<0, 4, false, true, kStgCells>(P, out_lens, in_mode, stream);
}
} // namespace lrp
