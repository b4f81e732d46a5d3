// lrp_camview_bc.hip — the bicubic instantiations of the camera-view kernel (lrp_camview_kernel.h; launcher:
// lrp_camview.hip).
#include <hip/hip_runtime.h>

#include "lrp_camview_kernel.h"

namespace lrp {

hipError_t launch_camera_view_bicubic(const CameraViewParams &P, hipStream_t stream) {
  return launch_camera_view_interp<2>(P, stream);
}

} // namespace lrp
