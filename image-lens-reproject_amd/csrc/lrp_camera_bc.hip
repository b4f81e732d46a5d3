// lrp_camera_bc.hip — the bicubic instantiations of the calibrated-camera compose kernel (lrp_camera_kernel.h; launcher:
// lrp_camera.hip).
#include <hip/hip_runtime.h>

#include "lrp_camera_kernel.h"

namespace lrp {

hipError_t launch_compose_cameras_bicubic(const CameraParams &P, int out_lens, hipStream_t stream) {
  return launch_compose_cameras_interp<2>(P, out_lens, stream);
}

} // namespace lrp
