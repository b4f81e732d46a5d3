// lrp_compose_bl.hip — the bilinear instantiations of the compose kernel (lrp_compose_kernel.h; launcher: lrp_compose.hip).
#include <hip/hip_runtime.h>

#include "lrp_compose_kernel.h"

namespace lrp {

hipError_t launch_compose_bilinear(const ComposeParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_compose_interp<1>(P, out_lens, in_mode, stream);
}

} // namespace lrp
