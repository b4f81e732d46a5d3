// lrp_camera_packed_bc_f16.hip — the bicubic instantiations of the packed camera compose kernel for half frames
// (lrp_camera_packed_kernel.h; launcher: lrp_camera_packed.hip).
#include <hip/hip_runtime.h>

#include "lrp_camera_packed_kernel.h"

namespace lrp {

hipError_t launch_camera_packed_bicubic_f16(const CameraPackedParams &P, int out_lens, hipStream_t stream) {
  return launch_camera_packed_fmt<2, kPackedF16>(P, out_lens, stream);
}

} // namespace lrp
