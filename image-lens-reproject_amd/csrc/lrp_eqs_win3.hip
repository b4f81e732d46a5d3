// lrp_eqs_win3.hip — window-kernel instantiations for the equisolid cells (lrp_eqs_win.h): 3 channels, one sample per pixel.
#include "lrp_eqs_win.h"

namespace lrp {
hipError_t launch_eqs_win_c3(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_eqs_win_impl<3, false>(P, out_lens, in_mode, stream);
}
} // namespace lrp
