// lrp_tile_unit.hip — the tile kernel's instantiations (lrp_kernel_v2.h) for the cells of one extension lens, per line of units.list:
//   -DLRP_INTERP=0|1|2  nearest, bilinear, bicubic
//   -DLRP_SET=1|2       the equisolid / the stereographic cells (lrp_cells.h CellSet)
// The cells of the reference's lenses are in the dispatchers' units, lrp_tile_{nn,bl,bc}.hip.
#if !defined(LRP_INTERP) || !defined(LRP_SET)
#error "lrp_tile_unit.hip: give -DLRP_INTERP=<0|1|2> and -DLRP_SET=<1|2> (units.list)"
#elif LRP_INTERP < 0 || LRP_INTERP > 2 || LRP_SET < 1 || LRP_SET > 2
#error "lrp_tile_unit.hip: LRP_INTERP 0..2, LRP_SET 1 (equisolid) or 2 (stereographic)"
#endif
#include "lrp_kernel_v2.h"

namespace lrp {
template <int Interp, CellSet Set> hipError_t launch_tile_unit(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_tile_interp<Interp, Set>(P, out_lens, in_mode, stream);
}
template hipError_t launch_tile_unit<LRP_INTERP, (CellSet)LRP_SET>(const KParams &, int, int, hipStream_t);
} // namespace lrp
