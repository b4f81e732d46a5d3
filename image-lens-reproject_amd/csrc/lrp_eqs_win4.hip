// lrp_eqs_win4.hip — bicubic window-kernel instantiations (lrp_kernel_v2.h): RGBA, plain blocks, the equisolid cells.
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_win_bicubic_c4_m0_eqs(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_win_bicubic_impl<0, 4, false, false, kEqsCells>(P, out_lens, in_mode, stream);
}
} // namespace lrp
