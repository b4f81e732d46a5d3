// lrp_compose_packed_bl.hip — the bilinear instantiations of the packed compose kernel (lrp_compose_packed_kernel.h; launcher:
// lrp_compose_packed.hip).
#include <hip/hip_runtime.h>

#include "lrp_compose_packed_kernel.h"

namespace lrp {

hipError_t launch_compose_packed_bilinear(const ComposePackedParams &P, int in_format, int out_lens, int in_mode, hipStream_t stream) {
  return launch_compose_packed_interp<1>(P, in_format, out_lens, in_mode, stream);
}

} // namespace lrp
