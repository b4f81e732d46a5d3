// lrp_compose.hip — several source images composed into one output by one launch (include/lrp.h "compose"):
// the launcher lrp_capi.cpp calls, and the nearest-neighbour instantiations of compose_kernel (lrp_compose_kernel.h).  The
// bilinear and bicubic ones are units of lrp_compose_unit.hip (units.list).
#include <hip/hip_runtime.h>

#include "lrp_compose_kernel.h"

namespace lrp {

// P: everything but the tiling.  interpolation: 0 nearest, 1 bilinear, 2 bicubic (include/lrp.h lrp_interpolation).
hipError_t launch_compose(const ComposeParams &P, int out_lens, int in_mode, int interpolation, hipStream_t stream) {
  if (P.n_src < 1 || P.n_src > kComposeMaxSources || P.ch_count < 1 || P.ch_count > kComposeMaxChannels) return hipErrorInvalidValue;
  if (interpolation == 0) return launch_compose_interp<0>(P, out_lens, in_mode, stream);
  if (interpolation == 1) return launch_compose_unit<1>(P, out_lens, in_mode, stream);
  if (interpolation == 2) return launch_compose_unit<2>(P, out_lens, in_mode, stream);
  return hipErrorInvalidValue;
}

} // namespace lrp
