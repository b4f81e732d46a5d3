// lrp_packed_bc.hip — the bicubic instantiations of the packed-pixel kernel (lrp_packed_kernel.h; launcher: lrp_packed.hip).
#include <hip/hip_runtime.h>

#include "lrp_packed_kernel.h"

namespace lrp {

hipError_t launch_packed_bicubic(const PackedParams &P, int in_format, int out_lens, int in_mode, hipStream_t stream) {
  return launch_packed_interp<2>(P, in_format, out_lens, in_mode, stream);
}

} // namespace lrp
