// lrp_compose_kernel.h — the compose kernel (include/lrp.h "compose"): several source images into one
// output, one launch.  Included by one unit per interpolation (lrp_compose.hip; lrp_compose_unit.hip twice, units.list)
// so that the three instantiation sets compile in parallel.
//
// Per output pixel: the target ray once; then, source by source, the rotation, ray_to_source and the coverage test of
// include/lrp.h "coverage" (what lrp_coverage.hip decides per sub-sample), a sample<> of the sources that cover the pixel, and
// one store.  No lens formula and no sampler is restated: target_ray, ray_to_source and sample<> are lrp_device.h's, the
// values — and the bits — those of the one-pixel-per-lane kernel (lrp_kernel_impl.h) for that source.  The per-pixel body
// itself is written twice: here, and in compose_packed_kernel (lrp_compose_packed_kernel.h) between other ends; folded onto
// one function, kernels of both moved registers.  The supersampled kernels share one body,
// lrp_compose_pixel.h, and take from here the tile, compose_min, LensSources and launch_compose_tiles.
//
// Mapping (gfx950): the 32 x 8 tile of lrp_kernel_impl.h, one pixel per lane, tiles in xcd_tile() order — this kernel reads
// sources, and neighbouring tiles share source rows in one XCD's L2.  The source loop is wave-uniform: its counter and the
// descriptor src[i] it selects from the kernarg block live in SGPRs (scalar loads), and a source that no active lane of the
// wavefront needs is skipped by a wave-wide test before any address is formed — in a cube-face job five of six.  FIRST leaves
// the loop once every active lane has a value.  No LDS; the channel count is the run-time Texel<0> path.
#pragma once

#include "lrp_cells.h"
#include "lrp_compose.h"
#include "lrp_device.h"

namespace lrp {

constexpr int kComposeTileW = 32;
constexpr int kComposeTileH = 8;
constexpr int kComposeThreads = kComposeTileW * kComposeTileH; // 256 = 4 wavefronts

using ComposeKernelFn = void (*)(const ComposeParams);
static_assert(kComposeMaxChannels == kMaxDynChannels && kComposeMaxSources == 8, "lrp_compose.h states the limits of lrp_device.h / include/lrp.h");

// The sources that fold a ray through x / -z (ray_to_source): a ray with vz >= 0 lands on the picture's mirrored ghost.
constexpr bool compose_folding_source(int in_mode) { return in_mode != kInEquirect && in_mode != kInEquirectLoop; }

// covered iff front && in_x && in_y (include/lrp.h "coverage"); comparisons with NaN are false.
template <int InMode> __device__ __forceinline__ bool compose_covered(float sx, float sy, float vz, float in_w, float in_h) {
  bool ok = sy >= -0.5f && sy <= in_h - 0.5f;
  if constexpr (InMode == kInEquirectLoop)
    ok = ok && sx == sx; // the wrapping sampler has a texel for every finite x
  else
    ok = ok && sx >= -0.5f && sx <= in_w - 0.5f;
  if constexpr (compose_folding_source(InMode)) ok = ok && vz < 0.0f;
  return ok;
}

// The sources of an ideal lens (the Sources policy of lrp_compose_pixel.h): ray_to_source and the coverage test.
template <int InMode> struct LensSources {
  static constexpr bool kLoop = (InMode == kInEquirectLoop);
  static __device__ __forceinline__ bool map(const ComposeSource &S, float vx, float vy, float vz, float in_w, float in_h, float &sx, float &sy) {
    float px, py;
    ray_to_source<InMode>(S.lens, in_w, in_h, vx, vy, vz, px, py);
    sx = (px - 0.5f) + in_w * 0.5f; // src/reproject.cpp:323-324
    sy = (py - 0.5f) + in_h * 0.5f;
    return compose_covered<InMode>(sx, sy, vz, in_w, in_h);
  }
};

// std::min: b where b < a
__device__ __forceinline__ float compose_min(float a, float b) { return (b < a) ? b : a; }

template <int OutLens, int InMode, int Interp>
__global__ __launch_bounds__(kComposeThreads) void compose_kernel(const ComposeParams P) {
  constexpr bool Loop = (InMode == kInEquirectLoop);
  constexpr int L = texel_lanes<0>();
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;

  // pixel centre and the one sub-sample of a num_samples == 1 call (src/reproject.cpp:287-298, as lrp_kernel_impl.h), then
  // the target ray, once for all sources
  const float scx = ((((float)x + 0.5f) - (float)P.out_w * 0.5f) + 0.5f) - 0.5f; // :295, (0 + 1) / (1 + 1) == 0.5f
  const float scy = ((((float)y + 0.5f) - (float)P.out_h * 0.5f) + 0.5f) - 0.5f; // :298
  float rx, ry, rz;
  target_ray<OutLens>(P.out_lens, (float)P.out_w, (float)P.out_h, scx, scy, rx, ry, rz);

  const int mode = P.mode;
  Texel<0> acc;
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  float wsum = 0.0f;
  uint32_t k = 0;

#pragma unroll 1
  for (int i = 0; i < P.n_src; ++i) {
    const ComposeSource &S = P.src[i]; // wave-uniform
    float vx = rx, vy = ry, vz = rz;
    if (S.has_rot) { // src/reproject.cpp:301-311
      vx = S.rot[0] * rx + S.rot[1] * ry + S.rot[2] * rz;
      vy = S.rot[3] * rx + S.rot[4] * ry + S.rot[5] * rz;
      vz = S.rot[6] * rx + S.rot[7] * ry + S.rot[8] * rz;
    }
    const float in_w = (float)S.in_w, in_h = (float)S.in_h;
    float px, py;
    ray_to_source<InMode>(S.lens, in_w, in_h, vx, vy, vz, px, py);
    const float sx = (px - 0.5f) + in_w * 0.5f; // src/reproject.cpp:323-324
    const float sy = (py - 0.5f) + in_h * 0.5f;
    const bool covered = compose_covered<InMode>(sx, sy, vz, in_w, in_h);
    const bool need = covered && (mode != kComposeFirst || k == 0u);
    if (__builtin_amdgcn_ballot_w64(need) != 0ull) { // a source no lane of the wavefront needs is not sampled
      if (need) {
        KParams Q; // the sampler's view of source i: sample<> reads these five fields of a KParams and nothing else
        Q.src = S.data;
        Q.in_w = S.in_w;
        Q.in_h = S.in_h;
        Q.channels = P.channels;
        Q.ch_count = P.ch_count;
        const Texel<0> s = sample<Interp, 0, Loop>(Q, sx, sy);
        if (mode == kComposeFeather) {
          const float dy = compose_min(sy + 0.5f, (in_h - 0.5f) - sy);
          float m = dy;
          if constexpr (!Loop) m = compose_min(compose_min(sx + 0.5f, (in_w - 0.5f) - sx), dy);
          const float w = (m < 0x1p-10f) ? 0x1p-10f : m;
#pragma unroll
          for (int c = 0; c < L; ++c) {
            const float t = w * s.v[c];
            acc.v[c] = acc.v[c] + t;
          }
          wsum = wsum + w;
        } else if (mode == kComposeMean) {
#pragma unroll
          for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] + s.v[c];
        } else {
#pragma unroll
          for (int c = 0; c < L; ++c) acc.v[c] = s.v[c];
        }
      }
    }
    k += covered ? 1u : 0u;
    // FIRST: every lane has its value (a count plane wants k of all sources)
    if (mode == kComposeFirst && P.count == nullptr && __builtin_amdgcn_ballot_w64(k == 0u) == 0ull) break;
  }

  if (k == 0u) { // no source covers the pixel: +0.0f in every channel, whatever post is
#pragma unroll
    for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  } else {
    if (mode != kComposeFirst) {
      const float div = mode == kComposeMean ? (float)k : wsum;
#pragma unroll
      for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] / div;
    }
    if (P.has_post) { // fused post_process: the first min(C, 3) channels (src/reproject.cpp:423-434)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c < P.ch_count) acc.v[c] = tonemap(acc.v[c], P.exposure, P.reinhard);
    }
  }
  const uint32_t px_index = (uint32_t)y * (uint32_t)P.out_w + (uint32_t)x;
  store_texel<0>(P.dst, px_index * (uint32_t)P.channels, acc, P.ch_count);
  if (P.count != nullptr) P.count[px_index] = (uint8_t)k;
}

// The cells of the compose kernel: all 30, per interpolation (the extension lenses are gated by the caller's validation).
// cell_kernel<> (lrp_cells.h) is a table of KernelFn — kernels that take a KParams; this kernel takes its own block, so it
// has a table of its own pointer type, over the same ids (kLensIds, kInModes, is_lens_id) and in the same layout: entry
// out_lens * kInModes + in_mode.
template <int Interp, int Cell> constexpr ComposeKernelFn compose_cell_entry() {
  if constexpr (is_lens_id(Cell / kInModes))
    return compose_kernel<Cell / kInModes, Cell % kInModes, Interp>;
  else
    return nullptr;
}
template <int Interp, int... Cell>
constexpr std::array<ComposeKernelFn, kLensIds * kInModes> compose_cell_table(std::integer_sequence<int, Cell...>) {
  return {{compose_cell_entry<Interp, Cell>()...}};
}
// The kernel of cell (out_lens, in_mode); nullptr: no such cell.
template <int Interp> ComposeKernelFn compose_cell_kernel(int out_lens, int in_mode) {
  static constexpr std::array<ComposeKernelFn, kLensIds * kInModes> table =
      compose_cell_table<Interp>(std::make_integer_sequence<int, kLensIds * kInModes>{});
  if (out_lens < 0 || out_lens >= kLensIds || in_mode < 0 || in_mode >= kInModes) return nullptr;
  return table[out_lens * kInModes + in_mode];
}

// Starts kernel fn over the 32 x 8 tiles of the output, with argument block A; P is the part of A that states out_w and out_h
// and takes tiles_x and tiles_y (A itself, or a block within it).  An empty output is no error; fn == nullptr: no such kernel.
template <typename Args, typename Block> hipError_t launch_compose_tiles(void (*fn)(const Args), Args &A, Block &P, hipStream_t stream) {
  P.tiles_x = (P.out_w + kComposeTileW - 1) / kComposeTileW;
  P.tiles_y = (P.out_h + kComposeTileH - 1) / kComposeTileH;
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  if (!fn) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, A);
  return hipGetLastError();
}

template <int Interp> hipError_t launch_compose_interp(ComposeParams P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_compose_tiles(compose_cell_kernel<Interp>(out_lens, in_mode), P, P, stream);
}

// ... as a bilinear / bicubic unit of units.list compiles it: defined and instantiated by lrp_compose_unit.hip, declared only for the launcher.
template <int Interp> hipError_t launch_compose_unit(const ComposeParams &P, int out_lens, int in_mode, hipStream_t stream);
} // namespace lrp
