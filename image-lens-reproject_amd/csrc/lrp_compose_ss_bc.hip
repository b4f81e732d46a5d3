// lrp_compose_ss_bc.hip — the bicubic instantiations of the supersampled compose kernel (lrp_compose_ss_kernel.h; launcher:
// lrp_compose_ss.hip).
#include <hip/hip_runtime.h>

#include "lrp_compose_ss_kernel.h"

namespace lrp {

hipError_t launch_compose_ss_bicubic(const ComposeSsParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_compose_ss_interp<2>(P, out_lens, in_mode, stream);
}

} // namespace lrp
