// lrp_camgain_bl.hip — the bilinear instantiations of the calibrated-camera compose kernel with gains (lrp_camgain_kernel.h;
// launcher: lrp_camgain.hip).
#include <hip/hip_runtime.h>

#include "lrp_camgain_kernel.h"

namespace lrp {

hipError_t launch_compose_cameras_gain_bilinear(const CameraGainParams &G, int out_lens, hipStream_t stream) {
  return launch_compose_cameras_gain_interp<1>(G, out_lens, stream);
}

} // namespace lrp
