// lrp_compose_packed_bc.hip — the bicubic instantiations of the packed compose kernel for 8-bit sources
// (lrp_compose_packed_kernel.h; launcher: lrp_compose_packed.hip).  Those for half sources are lrp_compose_packed_bc_f16.hip:
// one unit of all 120 would compile longest in the build.
#include <hip/hip_runtime.h>

#include "lrp_compose_packed_kernel.h"

namespace lrp {

hipError_t launch_compose_packed_bicubic_u8(const ComposePackedParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_compose_packed_fmt<2, kPackedU8>(P, out_lens, in_mode, stream);
}

} // namespace lrp
