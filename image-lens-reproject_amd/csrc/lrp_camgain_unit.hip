// lrp_camgain_unit.hip — the bilinear or the bicubic instantiations of the calibrated-camera compose kernel with gains
// (lrp_camgain_kernel.h; launcher and nearest: lrp_camgain.hip), per line of units.list:  -DLRP_INTERP=1|2
#if !defined(LRP_INTERP)
#error "lrp_camgain_unit.hip: give -DLRP_INTERP=<1 bilinear | 2 bicubic> (units.list)"
#elif LRP_INTERP < 1 || LRP_INTERP > 2
#error "lrp_camgain_unit.hip: LRP_INTERP 1 (bilinear) or 2 (bicubic); nearest is lrp_camgain.hip's own"
#endif
#include <hip/hip_runtime.h>

#include "lrp_camgain_kernel.h"

namespace lrp {

template <int Interp> hipError_t launch_compose_cameras_gain_unit(const CameraGainParams &G, int out_lens, hipStream_t stream) {
  return launch_compose_cameras_gain_interp<Interp>(G, out_lens, stream);
}
template hipError_t launch_compose_cameras_gain_unit<LRP_INTERP>(const CameraGainParams &, int, hipStream_t);

} // namespace lrp
