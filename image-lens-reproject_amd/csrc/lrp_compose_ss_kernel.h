// lrp_compose_ss_kernel.h — the supersampled compose kernel (include/lrp.h "compose, supersampled"):
// several source images into one output with n x n sub-samples per pixel, one launch.  Included by one unit per
// interpolation (lrp_compose_ss.hip; lrp_compose_ss_unit.hip twice, units.list) so that the three instantiation sets
// compile in parallel.
//
// Per output pixel: compose_ss_pixel (lrp_compose_pixel.h), the supersampled body, with the sources and the target of ideal
// lenses — LensSources<InMode> (lrp_compose_kernel.h) and IdealTarget<OutLens> — and no per-sample hook.  This header holds the
// kernel's name, its cells and its launcher; nothing of the body is restated.
//
// Mapping (gfx950): lrp_compose_pixel.h's; one instantiation set serves every n.
#pragma once

#include "lrp_compose_pixel.h"
#include "lrp_compose_ss.h"

namespace lrp {

using ComposeSsKernelFn = void (*)(const ComposeSsParams);

template <int OutLens, int InMode, int Interp>
__global__ __launch_bounds__(kComposeThreads) void compose_ss_kernel(const ComposeSsParams P) {
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;
  compose_ss_pixel<Interp, LensSources<InMode>, IdealTarget<OutLens>>(P, x, y, NoSampleHook{});
}

// The cells: all 30, per interpolation, in the layout of compose_cell_table (entry out_lens * kInModes + in_mode).
template <int Interp, int Cell> constexpr ComposeSsKernelFn compose_ss_cell_entry() {
  if constexpr (is_lens_id(Cell / kInModes))
    return compose_ss_kernel<Cell / kInModes, Cell % kInModes, Interp>;
  else
    return nullptr;
}
template <int Interp, int... Cell>
constexpr std::array<ComposeSsKernelFn, kLensIds * kInModes> compose_ss_cell_table(std::integer_sequence<int, Cell...>) {
  return {{compose_ss_cell_entry<Interp, Cell>()...}};
}
// The kernel of cell (out_lens, in_mode); nullptr: no such cell.
template <int Interp> ComposeSsKernelFn compose_ss_cell_kernel(int out_lens, int in_mode) {
  static constexpr std::array<ComposeSsKernelFn, kLensIds * kInModes> table =
      compose_ss_cell_table<Interp>(std::make_integer_sequence<int, kLensIds * kInModes>{});
  if (out_lens < 0 || out_lens >= kLensIds || in_mode < 0 || in_mode >= kInModes) return nullptr;
  return table[out_lens * kInModes + in_mode];
}

template <int Interp> hipError_t launch_compose_ss_interp(ComposeSsParams P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_compose_tiles(compose_ss_cell_kernel<Interp>(out_lens, in_mode), P, P, stream);
}

// ... as a bilinear / bicubic unit of units.list compiles it: defined and instantiated by lrp_compose_ss_unit.hip, declared only for the launcher.
template <int Interp> hipError_t launch_compose_ss_unit(const ComposeSsParams &P, int out_lens, int in_mode, hipStream_t stream);
} // namespace lrp
