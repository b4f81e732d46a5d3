// lrp_win_unit.hip — one set of bicubic window-kernel instantiations (lrp_kernel_v2.h) per line of units.list:
//   -DLRP_WIN_Q=0..4   mirror mode (lrp_win_kernel.h QMode: 0 plain blocks, 1 both axes, 2 rows, 3 columns, 4 shared rays)
//   -DLRP_WIN_C=3|4|5  channels (RGB, RGBA, RGBAZ)
//   -DLRP_WIN_GEO=1    coordinates from the geometry cache (GeoRead)                                 } plain blocks only;
//   -DLRP_WIN_SS=1     num_samples 2-4 (with LRP_WIN_GEO: from a geometry-cache entry of sub-samples) } absent: 0
//   -DLRP_WIN_SET=1|2  the equisolid / the stereographic cells (lrp_cells.h CellSet)                  }
// The plain RGBA unit is lrp_tile_win.hip, next to the dispatcher.
#ifndef LRP_WIN_GEO
#define LRP_WIN_GEO 0
#endif
#ifndef LRP_WIN_SS
#define LRP_WIN_SS 0
#endif
#ifndef LRP_WIN_SET
#define LRP_WIN_SET 0
#endif
#if !defined(LRP_WIN_Q) || !defined(LRP_WIN_C)
#error "lrp_win_unit.hip: give -DLRP_WIN_Q=<mirror mode 0..4> and -DLRP_WIN_C=<channels 3|4|5> (units.list)"
#elif LRP_WIN_Q < 0 || LRP_WIN_Q > 4 || LRP_WIN_C < 3 || LRP_WIN_C > 5 || LRP_WIN_GEO < 0 || LRP_WIN_GEO > 1 || LRP_WIN_SS < 0 || LRP_WIN_SS > 1 || LRP_WIN_SET < 0 || LRP_WIN_SET > 2
#error "lrp_win_unit.hip: LRP_WIN_Q 0..4, LRP_WIN_C 3..5, LRP_WIN_GEO 0|1, LRP_WIN_SS 0|1, LRP_WIN_SET 0..2"
#elif LRP_WIN_Q != 0 && (LRP_WIN_GEO || LRP_WIN_SS || LRP_WIN_SET)
#error "lrp_win_unit.hip: the geometry cache, supersampling and the extension lenses have plain blocks only (LRP_WIN_Q=0)"
#elif LRP_WIN_GEO && LRP_WIN_SET
#error "lrp_win_unit.hip: a launch that reads the geometry cache holds no lens math (lrp_cells.h launch_cell_set): LRP_WIN_SET=0"
#elif LRP_WIN_Q == 0 && LRP_WIN_C == 4 && !LRP_WIN_GEO && !LRP_WIN_SS && !LRP_WIN_SET
#error "lrp_win_unit.hip: the plain RGBA instantiations are lrp_tile_win.hip's own"
#endif
#include "lrp_kernel_v2.h"

namespace lrp {
template <int QMode, int CH, bool GeoRead, bool SS, CellSet Set>
hipError_t launch_win_unit(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_win_bicubic_impl<QMode, CH, GeoRead, SS, Set>(P, out_lens, in_mode, stream);
}
template hipError_t launch_win_unit<LRP_WIN_Q, LRP_WIN_C, LRP_WIN_GEO != 0, LRP_WIN_SS != 0, (CellSet)LRP_WIN_SET>(const KParams &, int, int, hipStream_t);
} // namespace lrp

#if defined(LRP_TIER_STATS) && LRP_WIN_Q == 1 && LRP_WIN_C == 4
extern "C" void lrp_debug_read_tiers(unsigned out[8]) { // mirrored RGBA instantiations only (lrp_tile_winq.o)
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(lrp::g_tier_stats), sizeof(unsigned) * 8);
  unsigned zero[8] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(lrp::g_tier_stats), zero, sizeof(zero));
}
#endif
#if defined(LRP_WAVE_STAMPS) && LRP_WIN_C == 4 && LRP_WIN_GEO && !LRP_WIN_SS
extern "C" void lrp_debug_read_wave_stamps(unsigned long long *out, int n_waves) { // (lrp_tile_wing.o: RGBA, coordinates from the geometry cache)
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(lrp::g_wave_stamps), sizeof(unsigned long long) * 3 * (size_t)n_waves);
}
#endif
