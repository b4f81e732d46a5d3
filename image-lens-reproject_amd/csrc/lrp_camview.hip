// lrp_camview.hip — frames of calibrated cameras composed into the frame of a calibrated target camera by one launch
// (include/lrp.h "calibrated camera as the target"): the launcher lrp_capi.cpp calls, and the
// nearest-neighbour instantiations of camera_view_kernel (lrp_camview_kernel.h).  The bilinear and bicubic ones are
// units of lrp_camview_unit.hip (units.list).
#include <hip/hip_runtime.h>

#include "lrp_camview_kernel.h"

namespace lrp {

// P: everything but the tiling.  interpolation: 0 nearest, 1 bilinear, 2 bicubic (include/lrp.h lrp_interpolation).
hipError_t launch_camera_view(const CameraViewParams &P, int interpolation, hipStream_t stream) {
  if (P.n_src < 1 || P.n_src > kComposeMaxSources || P.ch_count < 1 || P.ch_count > kComposeMaxChannels) return hipErrorInvalidValue;
  if (P.num_samples < 1 || P.num_samples > kComposeSsMaxSamples) return hipErrorInvalidValue;
  if (interpolation == 0) return launch_camera_view_interp<0>(P, stream);
  if (interpolation == 1) return launch_camera_view_unit<1>(P, stream);
  if (interpolation == 2) return launch_camera_view_unit<2>(P, stream);
  return hipErrorInvalidValue;
}

} // namespace lrp
