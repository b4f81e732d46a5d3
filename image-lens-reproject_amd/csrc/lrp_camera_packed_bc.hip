// lrp_camera_packed_bc.hip — the bicubic instantiations of the packed camera compose kernel for 8-bit frames
// (lrp_camera_packed_kernel.h; launcher: lrp_camera_packed.hip).  Those for half frames are lrp_camera_packed_bc_f16.hip: one
// unit of all twenty would compile among the longest in the build.
#include <hip/hip_runtime.h>

#include "lrp_camera_packed_kernel.h"

namespace lrp {

hipError_t launch_camera_packed_bicubic_u8(const CameraPackedParams &P, int out_lens, hipStream_t stream) {
  return launch_camera_packed_fmt<2, kPackedU8>(P, out_lens, stream);
}

} // namespace lrp
