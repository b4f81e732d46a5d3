// lrp_eqs_wins5.hip — window-kernel instantiations for the equisolid cells (lrp_eqs_win.h): 5 channels, num_samples 2-4.
#include "lrp_eqs_win.h"

namespace lrp {
hipError_t launch_eqs_win_ss_c5(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_eqs_win_impl<5, true>(P, out_lens, in_mode, stream);
}
} // namespace lrp
