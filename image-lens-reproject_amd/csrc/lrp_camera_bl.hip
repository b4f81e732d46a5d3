// lrp_camera_bl.hip — the bilinear instantiations of the calibrated-camera compose kernel (lrp_camera_kernel.h; launcher:
// lrp_camera.hip).
#include <hip/hip_runtime.h>

#include "lrp_camera_kernel.h"

namespace lrp {

hipError_t launch_compose_cameras_bilinear(const CameraParams &P, int out_lens, hipStream_t stream) {
  return launch_compose_cameras_interp<1>(P, out_lens, stream);
}

} // namespace lrp
