// lrp_compose_packed_bc_f16.hip — the bicubic instantiations of the packed compose kernel for half sources
// (lrp_compose_packed_kernel.h; launcher: lrp_compose_packed.hip).
#include <hip/hip_runtime.h>

#include "lrp_compose_packed_kernel.h"

namespace lrp {

hipError_t launch_compose_packed_bicubic_f16(const ComposePackedParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_compose_packed_fmt<2, kPackedF16>(P, out_lens, in_mode, stream);
}

} // namespace lrp
