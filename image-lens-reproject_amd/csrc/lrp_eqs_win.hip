// lrp_eqs_win.hip — the window-kernel dispatcher of the equisolid cells (lrp_eqs.h).
#include "lrp_eqs.h"

namespace lrp {
hipError_t launch_eqs_win_c3(const KParams &P, int out_lens, int in_mode, hipStream_t stream);    // lrp_eqs_win3.hip
hipError_t launch_eqs_win_c4(const KParams &P, int out_lens, int in_mode, hipStream_t stream);    // lrp_eqs_win4.hip
hipError_t launch_eqs_win_c5(const KParams &P, int out_lens, int in_mode, hipStream_t stream);    // lrp_eqs_win5.hip
hipError_t launch_eqs_win_ss_c3(const KParams &P, int out_lens, int in_mode, hipStream_t stream); // lrp_eqs_wins3.hip
hipError_t launch_eqs_win_ss_c4(const KParams &P, int out_lens, int in_mode, hipStream_t stream); // lrp_eqs_wins4.hip
hipError_t launch_eqs_win_ss_c5(const KParams &P, int out_lens, int in_mode, hipStream_t stream); // lrp_eqs_wins5.hip
// P.channels 3, 4 or 5, P.num_samples 1 to 4, P.win_mode 0, P.geo_mode 0 / 1 (1: the single launch writes the entry).
namespace {
hipError_t launch_eqs_win_bicubic(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  using Fn = hipError_t (*)(const KParams &, int, int, hipStream_t);
  static const Fn plain[3] = {launch_eqs_win_c3, launch_eqs_win_c4, launch_eqs_win_c5};
  static const Fn ss[3] = {launch_eqs_win_ss_c3, launch_eqs_win_ss_c4, launch_eqs_win_ss_c5};
  if (P.channels < 3 || P.channels > 5 || P.win_mode != 0 || P.geo_mode == 2) return hipErrorInvalidValue;
  return (P.num_samples >= 2 ? ss : plain)[P.channels - 3](P, out_lens, in_mode, stream);
}
const bool g_registered = (g_eqs_launchers.win = launch_eqs_win_bicubic, true);
} // namespace
} // namespace lrp
