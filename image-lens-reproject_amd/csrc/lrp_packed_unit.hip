// lrp_packed_unit.hip — the bilinear or the bicubic instantiations of the packed-pixel kernel (lrp_packed_kernel.h; launcher
// and nearest: lrp_packed.hip), per line of units.list:  -DLRP_INTERP=1|2
#if !defined(LRP_INTERP)
#error "lrp_packed_unit.hip: give -DLRP_INTERP=<1 bilinear | 2 bicubic> (units.list)"
#elif LRP_INTERP < 1 || LRP_INTERP > 2
#error "lrp_packed_unit.hip: LRP_INTERP 1 (bilinear) or 2 (bicubic); nearest is lrp_packed.hip's own"
#endif
#include <hip/hip_runtime.h>

#include "lrp_packed_kernel.h"

namespace lrp {

template <int Interp> hipError_t launch_packed_unit(const PackedParams &P, int in_format, int out_lens, int in_mode, hipStream_t stream) {
  return launch_packed_interp<Interp>(P, in_format, out_lens, in_mode, stream);
}
template hipError_t launch_packed_unit<LRP_INTERP>(const PackedParams &, int, int, int, hipStream_t);

} // namespace lrp
