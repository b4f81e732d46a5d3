// lrp_pixel_unit.hip — the reprojection kernel's instantiations (lrp_kernel_impl.h) for the cells of one extension lens, three
// samplers, per line of units.list:
//   -DLRP_SET=1|2  the equisolid / the stereographic cells (lrp_cells.h CellSet)
// The cells of the reference's lenses are in the dispatchers' units, lrp_kernels_{nn,bl,bc}.hip.
#if !defined(LRP_SET)
#error "lrp_pixel_unit.hip: give -DLRP_SET=<1|2> (units.list)"
#elif LRP_SET < 1 || LRP_SET > 2
#error "lrp_pixel_unit.hip: LRP_SET 1 (equisolid) or 2 (stereographic)"
#endif
#include "lrp_kernel_impl.h"

namespace lrp {
template <int Interp, CellSet Set> hipError_t launch_pixel_unit(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_interp<Interp, Set>(P, out_lens, in_mode, stream);
}
template hipError_t launch_pixel_unit<0, (CellSet)LRP_SET>(const KParams &, int, int, hipStream_t);
template hipError_t launch_pixel_unit<1, (CellSet)LRP_SET>(const KParams &, int, int, hipStream_t);
template hipError_t launch_pixel_unit<2, (CellSet)LRP_SET>(const KParams &, int, int, hipStream_t);
} // namespace lrp
