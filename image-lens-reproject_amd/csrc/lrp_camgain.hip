// lrp_camgain.hip — frames of calibrated cameras composed with one gain per camera (include/lrp.h "exposure matching across a
// camera rig"): the launcher lrp_capi.cpp calls, and the nearest-neighbour instantiations of
// camgain_kernel (lrp_camgain_kernel.h).  The bilinear and bicubic ones are units of lrp_camgain_unit.hip (units.list).
#include <hip/hip_runtime.h>

#include "lrp_camgain_kernel.h"

namespace lrp {

// G: everything but the tiling.  interpolation: 0 nearest, 1 bilinear, 2 bicubic (include/lrp.h lrp_interpolation).
hipError_t launch_compose_cameras_gain(const CameraGainParams &G, int out_lens, int interpolation, hipStream_t stream) {
  const CameraParams &P = G.cam;
  if (P.n_src < 1 || P.n_src > kComposeMaxSources || P.ch_count < 1 || P.ch_count > kComposeMaxChannels) return hipErrorInvalidValue;
  if (P.num_samples < 1 || P.num_samples > kComposeSsMaxSamples) return hipErrorInvalidValue;
  if (interpolation == 0) return launch_compose_cameras_gain_interp<0>(G, out_lens, stream);
  if (interpolation == 1) return launch_compose_cameras_gain_unit<1>(G, out_lens, stream);
  if (interpolation == 2) return launch_compose_cameras_gain_unit<2>(G, out_lens, stream);
  return hipErrorInvalidValue;
}

} // namespace lrp
