// lrp_camera_unit.hip — the bilinear or the bicubic instantiations of the calibrated-camera compose kernel
// (lrp_camera_kernel.h; launcher and nearest: lrp_camera.hip), per line of units.list:  -DLRP_INTERP=1|2
#if !defined(LRP_INTERP)
#error "lrp_camera_unit.hip: give -DLRP_INTERP=<1 bilinear | 2 bicubic> (units.list)"
#elif LRP_INTERP < 1 || LRP_INTERP > 2
#error "lrp_camera_unit.hip: LRP_INTERP 1 (bilinear) or 2 (bicubic); nearest is lrp_camera.hip's own"
#endif
#include <hip/hip_runtime.h>

#include "lrp_camera_kernel.h"

namespace lrp {

template <int Interp> hipError_t launch_compose_cameras_unit(const CameraParams &P, int out_lens, hipStream_t stream) {
  return launch_compose_cameras_interp<Interp>(P, out_lens, stream);
}
template hipError_t launch_compose_cameras_unit<LRP_INTERP>(const CameraParams &, int, hipStream_t);

} // namespace lrp
