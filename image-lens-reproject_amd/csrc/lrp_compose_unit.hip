// lrp_compose_unit.hip — the bilinear or the bicubic instantiations of the compose kernel (lrp_compose_kernel.h; launcher and
// nearest: lrp_compose.hip), per line of units.list:  -DLRP_INTERP=1|2
#if !defined(LRP_INTERP)
#error "lrp_compose_unit.hip: give -DLRP_INTERP=<1 bilinear | 2 bicubic> (units.list)"
#elif LRP_INTERP < 1 || LRP_INTERP > 2
#error "lrp_compose_unit.hip: LRP_INTERP 1 (bilinear) or 2 (bicubic); nearest is lrp_compose.hip's own"
#endif
#include <hip/hip_runtime.h>

#include "lrp_compose_kernel.h"

namespace lrp {

template <int Interp> hipError_t launch_compose_unit(const ComposeParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_compose_interp<Interp>(P, out_lens, in_mode, stream);
}
template hipError_t launch_compose_unit<LRP_INTERP>(const ComposeParams &, int, int, hipStream_t);

} // namespace lrp
