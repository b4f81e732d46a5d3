// lrp_camview_unit.hip — the bilinear or the bicubic instantiations of the camera-view kernel (lrp_camview_kernel.h; launcher
// and nearest: lrp_camview.hip), per line of units.list:  -DLRP_INTERP=1|2
#if !defined(LRP_INTERP)
#error "lrp_camview_unit.hip: give -DLRP_INTERP=<1 bilinear | 2 bicubic> (units.list)"
#elif LRP_INTERP < 1 || LRP_INTERP > 2
#error "lrp_camview_unit.hip: LRP_INTERP 1 (bilinear) or 2 (bicubic); nearest is lrp_camview.hip's own"
#endif
#include <hip/hip_runtime.h>

#include "lrp_camview_kernel.h"

namespace lrp {

template <int Interp> hipError_t launch_camera_view_unit(const CameraViewParams &P, hipStream_t stream) {
  return launch_camera_view_interp<Interp>(P, stream);
}
template hipError_t launch_camera_view_unit<LRP_INTERP>(const CameraViewParams &, hipStream_t);

} // namespace lrp
