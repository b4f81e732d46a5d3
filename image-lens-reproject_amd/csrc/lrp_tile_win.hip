// lrp_tile_win.hip — bicubic window-kernel instantiations (lrp_kernel_v2.h): RGBA, plain blocks; the dispatcher.
#include "lrp_kernel_v2.h"

namespace lrp {
// This unit's own instantiations: RGBA, plain blocks.  Every other (mirror mode, channel count, GeoRead, SS, cell set) is a
// line of units.list that compiles lrp_win_unit.hip; they compile in parallel.
template <> hipError_t launch_win_unit<0, 4>(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_win_bicubic_impl<0, 4>(P, out_lens, in_mode, stream);
}
// ... by channel count: RGB, RGBA, RGBAZ
using WinUnitFn = hipError_t (*)(const KParams &, int, int, hipStream_t);
template <int QMode, bool GeoRead = false, bool SS = false, CellSet Set = kStdCells>
constexpr WinUnitFn kWinUnits[3] = {launch_win_unit<QMode, 3, GeoRead, SS, Set>, launch_win_unit<QMode, 4, GeoRead, SS, Set>, launch_win_unit<QMode, 5, GeoRead, SS, Set>};

// P.channels must be 3, 4 or 5, P.num_samples 1 to 4; P.win_mode = the mirror mode (lrp_kernel_v2.h QMode).
// P.geo_mode == 2: the instantiations that load their coordinates from the geometry cache (plain blocks).
// P.num_samples 2, 3, 4: the supersampling instantiations (plain blocks; P.geo_mode 1 / 2: they write / read an entry of sub-samples).
// The cells with an equisolid or a stereographic lens (lrp_cells.h kEqsCells, kStgCells): plain blocks only, units of their own.
hipError_t launch_win_bicubic(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  const CellSet set = launch_cell_set(P, out_lens, in_mode);
  const bool eqs = set == kEqsCells, stg = set == kStgCells;
  if (P.num_samples >= 2) {
    if (P.win_mode != 0 || P.geo_mode == 3) return hipErrorInvalidValue;
    return (P.geo_mode == 2 ? kWinUnits<0, true, true> // (2: the entry of sub-samples is read)
            : eqs           ? kWinUnits<0, false, true, kEqsCells>
            : stg           ? kWinUnits<0, false, true, kStgCells>
                            : kWinUnits<0, false, true>)[P.channels - 3](P, out_lens, in_mode, stream);
  }
  if (P.geo_mode == 2) {
    if (P.win_mode != 0) return hipErrorInvalidValue;
    return kWinUnits<0, true>[P.channels - 3](P, out_lens, in_mode, stream);
  }
  static constexpr const WinUnitFn *by_mode[5] = {kWinUnits<0>, kWinUnits<1>, kWinUnits<2>, kWinUnits<3>, kWinUnits<4>};
  if (P.win_mode < 0 || P.win_mode > 4) return hipErrorInvalidValue;
  if (eqs && P.win_mode == 0) return kWinUnits<0, false, false, kEqsCells>[P.channels - 3](P, out_lens, in_mode, stream);
  if (stg && P.win_mode == 0) return kWinUnits<0, false, false, kStgCells>[P.channels - 3](P, out_lens, in_mode, stream);
  return by_mode[P.win_mode][P.channels - 3](P, out_lens, in_mode, stream);
}
} // namespace lrp

#if defined(LRP_TIER_STATS)
extern "C" void lrp_debug_read_tiers_plain(unsigned out[8]) { // plain RGBA instantiations only
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(lrp::g_tier_stats), sizeof(unsigned) * 8);
  unsigned zero[8] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(lrp::g_tier_stats), zero, sizeof(zero));
}
#endif
