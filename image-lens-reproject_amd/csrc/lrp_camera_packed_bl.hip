// lrp_camera_packed_bl.hip — the bilinear instantiations of the packed camera compose kernel (lrp_camera_packed_kernel.h;
// launcher: lrp_camera_packed.hip).
#include <hip/hip_runtime.h>

#include "lrp_camera_packed_kernel.h"

namespace lrp {

hipError_t launch_camera_packed_bilinear(const CameraPackedParams &P, int in_format, int out_lens, hipStream_t stream) {
  return launch_camera_packed_interp<1>(P, in_format, out_lens, stream);
}

} // namespace lrp
