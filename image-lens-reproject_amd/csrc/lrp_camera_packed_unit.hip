// lrp_camera_packed_unit.hip — the bilinear or the bicubic instantiations of the packed camera compose kernel
// (lrp_camera_packed_kernel.h; launcher and nearest: lrp_camera_packed.hip), per line of units.list:
//   -DLRP_INTERP=1|2    bilinear, bicubic
//   -DLRP_FORMAT=0|1|2  the frames' formats: 0 both, 1 half, 2 8-bit (lrp_packed.h kPackedF16, kPackedU8).  The bicubic
//                       instantiations are split by format: one unit of all twenty would compile among the longest in the build.
#if !defined(LRP_INTERP) || !defined(LRP_FORMAT)
#error "lrp_camera_packed_unit.hip: give -DLRP_INTERP=<1 bilinear | 2 bicubic> and -DLRP_FORMAT=<0 both | 1 half | 2 8-bit> (units.list)"
#elif LRP_INTERP < 1 || LRP_INTERP > 2 || LRP_FORMAT < 0 || LRP_FORMAT > 2
#error "lrp_camera_packed_unit.hip: LRP_INTERP 1 or 2 (nearest is lrp_camera_packed.hip's own), LRP_FORMAT 0, 1 or 2"
#endif
#include <hip/hip_runtime.h>

#include "lrp_camera_packed_kernel.h"

namespace lrp {

template <int Interp, int Fmt> hipError_t launch_camera_packed_unit(const CameraPackedParams &P, int out_lens, hipStream_t stream) {
  return launch_camera_packed_fmt<Interp, Fmt>(P, out_lens, stream);
}
#if LRP_FORMAT == 0 || LRP_FORMAT == 2
template hipError_t launch_camera_packed_unit<LRP_INTERP, kPackedU8>(const CameraPackedParams &, int, hipStream_t);
#endif
#if LRP_FORMAT == 0 || LRP_FORMAT == 1
template hipError_t launch_camera_packed_unit<LRP_INTERP, kPackedF16>(const CameraPackedParams &, int, hipStream_t);
#endif

} // namespace lrp
