// lrp_lanczos_kernel.h — the kernels of the Lanczos-3 sampler (include/lrp.h "Lanczos-3").
//
//   lanczos_kernel       computes: the pixel kernel's shape (lrp_kernel_impl.h) — a 32 x 8 tile, one pixel per lane, tiles in
//                        xcd_tile() order, the num_samples loop — with sample_lanczos; P.geo_mode == 1 also stores (sx, sy)
//                        into the geometry-cache entry.  One instantiation per cell (lrp_lanczos.hip).
//   lanczos_geo_kernel   reads the entry (P.geo_mode == 2): no lens math, one instantiation per <Loop, CH>
//                        (lrp_lanczos_geo.hip).
//
// Both gather their 36 taps per lane.  A variant of the RGBA lanczos_geo_kernel that staged the source window of its tile in
// LDS was measured slower than the gather on both benchmark geometries and is not kept: the kernels
// are bound by the arithmetic of the weights — eight sines / cosines and 32 IEEE divisions per pixel —, not by their taps.
#pragma once

#include "lrp_cells.h"
#include "lrp_lanczos.h"

namespace lrp {

constexpr int kLzTileW = 32;
constexpr int kLzTileH = 8;
constexpr int kLzThreads = kLzTileW * kLzTileH; // 256 = 4 wavefronts

template <int OutLens, int InMode, int CH>
__global__ __launch_bounds__(kLzThreads) void lanczos_kernel(const KParams P) {
  constexpr bool Loop = (InMode == kInEquirectLoop);
  constexpr int L = texel_lanes<CH>();
  typedef float vf2 __attribute__((ext_vector_type(2)));
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kLzTileW + (int)(threadIdx.x % kLzTileW);
  const int y = P.y_offset + ty * kLzTileH + (int)(threadIdx.x / kLzTileW);
  if (x >= P.out_w || y >= P.y_end) return;

  const float cx = ((float)x + 0.5f) - (float)P.out_w * 0.5f;
  const float cy = ((float)y + 0.5f) - (float)P.out_h * 0.5f;
  Texel<CH> acc;
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  const int ns = P.num_samples;
  const float ns1 = (float)ns + 1.0f;
  for (int ssx = 0; ssx < ns; ++ssx) {
    const float scx = cx + ((float)ssx + 1.0f) / ns1 - 0.5f;
    for (int ssy = 0; ssy < ns; ++ssy) {
      const float scy = cy + ((float)ssy + 1.0f) / ns1 - 0.5f;
      float sx, sy;
      source_position<OutLens, InMode>(P, scx, scy, sx, sy);
      if (P.geo_mode == 1) reinterpret_cast<vf2 *>(P.geo_xy)[geo_map_index(x, y, P.out_w)] = vf2{sx, sy}; // (num_samples == 1)
      const Texel<CH> s = sample_lanczos<CH, Loop>(P, sx, sy);
#pragma unroll
      for (int c = 0; c < L; ++c) acc.v[c] += s.v[c];
    }
  }
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] * P.normalize;
  if (P.has_post) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < L && c < P.ch_count) acc.v[c] = tonemap(acc.v[c], P.exposure, P.reinhard);
  }
  const uint32_t off = ((uint32_t)y * (uint32_t)P.out_w + (uint32_t)x) * (uint32_t)P.channels;
  store_texel<CH>(P.dst, off, acc, P.ch_count);
}

// The cells of the computing kernel: all 30 (the extension lenses are gated by the caller's validation).
template <int CH> struct LanczosCell {
  template <int OutLens, int InMode> static constexpr KernelFn kernel() { return lanczos_kernel<OutLens, InMode, CH>; }
};

// Whole images only (the entry has no bands), num_samples == 1.
template <bool Loop, int CH>
__global__ __launch_bounds__(kLzThreads) void lanczos_geo_kernel(const KParams P) {
  constexpr int L = texel_lanes<CH>();
  typedef float vf2 __attribute__((ext_vector_type(2)));
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kLzTileW + (int)(threadIdx.x % kLzTileW);
  const int y = P.y_offset + ty * kLzTileH + (int)(threadIdx.x / kLzTileW);
  if (x >= P.out_w || y >= P.y_end) return;
  const vf2 xy = reinterpret_cast<const vf2 *>(P.geo_xy)[geo_map_index(x, y, P.out_w)];
  Texel<CH> acc = sample_lanczos<CH, Loop>(P, xy.x, xy.y);
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = 0.0f + acc.v[c]; // acc = 0; acc += s, as the computing kernel accumulates
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] * P.normalize;
  if (P.has_post) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < L && c < P.ch_count) acc.v[c] = tonemap(acc.v[c], P.exposure, P.reinhard);
  }
  store_texel<CH>(P.dst, ((uint32_t)y * (uint32_t)P.out_w + (uint32_t)x) * (uint32_t)P.channels, acc, P.ch_count);
}

// The grid of a launch over rows [y_offset, y_end) of P; false: nothing to render.
inline bool lanczos_grid(KParams &P, dim3 &grid) {
  P.tiles_x = (P.out_w + kLzTileW - 1) / kLzTileW;
  P.tiles_y = (P.y_end - P.y_offset + kLzTileH - 1) / kLzTileH;
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return false;
  grid = dim3((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x));
  return true;
}

} // namespace lrp
