// lrp_multiband_kernel.h — the pyramid kernels of multi-band blending (include/lrp.h "multi-band blending across a camera rig",
// DESIGN.md section 22): reduce, Laplacian-accumulate and collapse, each templated on the colour channel count C = 1 .. 4.
// Included by lrp_multiband.hip alone.  Binary32, un-fused, in the order the header writes; the sums over the cameras are
// read-modify-write in launch order on one stream — no atomics, the order is part of the definition.
//
// Mapping (gfx950), all three: 256 threads on a 32 x 8 tile of the level the kernel writes, one texel per lane, a plain 2-D
// grid (the kernels stream planes; no tile shares rows with a distant one).  A texel of C == 4 floats moves as one 16-byte
// access per lane.  Every index that leaves the level is bent back by the level's rule (clamp, or modulo w in x for a
// full-turn target) while the LDS window is filled, so the passes that follow index the window only.
//   reduce    the fine window 67 x 19 of a coarse tile with its 2-texel halo -> LDS, planar (C colour planes and the weight
//             plane), even columns first so that the 5 taps of neighbouring lanes are neighbouring words (ds_read_b32,
//             conflict-free; the fill's stores are 2-way, which a ds_write_b32 does not pay for); the horizontal pass 32 x 19
//             -> LDS; the vertical pass from LDS to the lane's registers.  (C + 1) x 7600 bytes.
//   expand    (Laplacian-accumulate and collapse) the coarse window 18 x 6 of a fine tile with its 1-texel halo -> LDS; the
//             horizontal pass 32 x 6 -> LDS; the vertical pass per lane.  C x 1200 bytes; the weight plane is not expanded.
#pragma once

#include <hip/hip_runtime.h>

#include "lrp_device.h" // tonemap
#include "lrp_multiband.h"

namespace lrp {

__device__ __forceinline__ int mb_clamp(int j, int n) { return j < 0 ? 0 : (j >= n ? n - 1 : j); }
// X_k(j): j modulo w, non-negative, for a wrapping target; else the clamp
__device__ __forceinline__ int mb_index_x(int j, int w, int wrap) {
  if (wrap) {
    const int r = j % w;
    return r < 0 ? r + w : r;
  }
  return mb_clamp(j, w);
}

template <int C> __device__ __forceinline__ void mb_load(const float *p, size_t texel, float (&v)[C]) {
  if constexpr (C == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(p + texel * 4); // (every plane starts at a multiple of 256 bytes)
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = p[texel * C + c];
  }
}
template <int C> __device__ __forceinline__ void mb_store(float *p, size_t texel, const float (&v)[C]) {
  if (C == 4 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0u) { // (wave-uniform: the caller's output may start at any float)
    *reinterpret_cast<float4 *>(p + texel * 4) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) p[texel * C + c] = v[c];
  }
}

// M_k of a texel: the plane, or at level 0 the label
__device__ __forceinline__ float mb_weight(const float *m, const uint8_t *label, int cam, size_t texel) {
  if (m != nullptr) return m[texel];
  return (int)label[texel] == cam ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------- reduce: level k -> k + 1
template <int C> __global__ __launch_bounds__(kMbThreads) void multiband_reduce_kernel(const MultibandReduceParams P) {
  __shared__ float raw[C + 1][kMbReduceRows][kMbReducePitch];
  __shared__ float hor[C + 1][kMbReduceRows][kMbTileW];
  static_assert(sizeof(raw) + sizeof(hor) == (size_t)mb_reduce_lds_bytes(C), "the LDS the design states");
  const int X0 = (int)blockIdx.x * kMbTileW, Y0 = (int)blockIdx.y * kMbTileH; // of the coarse level
  const int fx0 = 2 * X0 - 2, fy0 = 2 * Y0 - 2;                               // the window's corner in the fine level

  for (int t = (int)threadIdx.x; t < kMbReduceRows * kMbReduceCols; t += kMbThreads) {
    const int r = t / kMbReduceCols, j = t - r * kMbReduceCols;
    const int gx = mb_index_x(fx0 + j, P.w, P.wrap), gy = mb_clamp(fy0 + r, P.h);
    const size_t at = (size_t)gy * (size_t)P.w + (size_t)gx;
    float v[C];
    mb_load<C>(P.g, at, v);
    const int slot = (j & 1) * kMbReduceHalf + (j >> 1);
#pragma unroll
    for (int c = 0; c < C; ++c) raw[c][r][slot] = v[c];
    raw[C][r][slot] = mb_weight(P.m, P.label, P.cam, at);
  }
  __syncthreads();

  for (int t = (int)threadIdx.x; t < kMbReduceRows * kMbTileW; t += kMbThreads) {
    const int r = t / kMbTileW, xl = t % kMbTileW; // window column of tap d: 2 xl + 2 + d
#pragma unroll
    for (int c = 0; c <= C; ++c) {
      const float *row = raw[c][r];
      const float pm2 = row[xl], p0 = row[xl + 1], p2 = row[xl + 2];
      const float pm1 = row[kMbReduceHalf + xl], p1 = row[kMbReduceHalf + xl + 1];
      hor[c][r][xl] = (((pm2 + p2) + 4.0f * (pm1 + p1)) + 6.0f * p0) * 0.0625f;
    }
  }
  __syncthreads();

  const int xl = (int)threadIdx.x % kMbTileW, yl = (int)threadIdx.x / kMbTileW;
  const int x = X0 + xl, y = Y0 + yl;
  if (x >= P.cw || y >= P.ch) return;
  float out[C + 1];
#pragma unroll
  for (int c = 0; c <= C; ++c) {
    const float pm2 = hor[c][2 * yl][xl], pm1 = hor[c][2 * yl + 1][xl], p0 = hor[c][2 * yl + 2][xl];
    const float p1 = hor[c][2 * yl + 3][xl], p2 = hor[c][2 * yl + 4][xl];
    out[c] = (((pm2 + p2) + 4.0f * (pm1 + p1)) + 6.0f * p0) * 0.0625f;
  }
  const size_t at = (size_t)y * (size_t)P.cw + (size_t)x;
  float g[C];
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = out[c];
  mb_store<C>(P.cg, at, g);
  P.cm[at] = out[C];
}

// ---------------------------------------------------------------- expand: E(T) of this lane's texel of the fine tile
// T: the coarse level, cw x ch x C.  Every thread of the workgroup calls it (two barriers).
template <int C>
__device__ __forceinline__ void mb_expand(const float *T, int cw, int ch, int wrap, float (&coarse)[C][kMbExpandRows][kMbExpandCols],
                                          float (&hor)[C][kMbExpandRows][kMbTileW], float (&e)[C]) {
  const int cx0 = ((int)blockIdx.x * kMbTileW) / 2 - 1, cy0 = ((int)blockIdx.y * kMbTileH) / 2 - 1; // the window's corner
  const int t = (int)threadIdx.x;
  if (t < kMbExpandRows * kMbExpandCols) {
    const int r = t / kMbExpandCols, j = t - r * kMbExpandCols;
    const int gx = mb_index_x(cx0 + j, cw, wrap), gy = mb_clamp(cy0 + r, ch);
    float v[C];
    mb_load<C>(T, (size_t)gy * (size_t)cw + (size_t)gx, v);
#pragma unroll
    for (int c = 0; c < C; ++c) coarse[c][r][j] = v[c];
  }
  __syncthreads();
  if (t < kMbExpandRows * kMbTileW) {
    const int r = t / kMbTileW, xl = t % kMbTileW;
    const int il = (xl >> 1) + 1; // window column of c(i), i = x >> 1 (the tile starts at an even x)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float *row = coarse[c][r];
      hor[c][r][xl] = (xl & 1) ? (row[il] + row[il + 1]) * 0.5f : ((row[il - 1] + row[il + 1]) + 6.0f * row[il]) * 0.125f;
    }
  }
  __syncthreads();
  const int xl = t % kMbTileW, yl = t / kMbTileW;
  const int rl = (yl >> 1) + 1;
#pragma unroll
  for (int c = 0; c < C; ++c)
    e[c] = (yl & 1) ? (hor[c][rl][xl] + hor[c][rl + 1][xl]) * 0.5f : ((hor[c][rl - 1][xl] + hor[c][rl + 1][xl]) + 6.0f * hor[c][rl][xl]) * 0.125f;
}

// ---------------------------------------------------------------- Laplacian-accumulate: one camera into A_k, S_k
template <int C> __global__ __launch_bounds__(kMbThreads) void multiband_lap_kernel(const MultibandLapParams P) {
  __shared__ float coarse[C][kMbExpandRows][kMbExpandCols];
  __shared__ float hor[C][kMbExpandRows][kMbTileW];
  static_assert(sizeof(coarse) + sizeof(hor) == (size_t)mb_expand_lds_bytes(C), "the LDS the design states");
  float e[C];
#pragma unroll
  for (int c = 0; c < C; ++c) e[c] = 0.0f;
  if (!P.top) mb_expand<C>(P.cg, P.cw, P.ch, P.wrap, coarse, hor, e); // (kernel-uniform)
  const int x = (int)blockIdx.x * kMbTileW + (int)threadIdx.x % kMbTileW;
  const int y = (int)blockIdx.y * kMbTileH + (int)threadIdx.x / kMbTileW;
  if (x >= P.w || y >= P.h) return;
  const size_t at = (size_t)y * (size_t)P.w + (size_t)x;
  float g[C], a[C];
  mb_load<C>(P.g, at, g);
  const float m = mb_weight(P.m, P.label, P.cam, at);
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) a[c] = 0.0f;
  if (!P.first) {
    mb_load<C>(P.a, at, a);
    s = P.s[at];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float l = P.top ? g[c] : g[c] - e[c];
    const float t = (m == 0.0f) ? 0.0f : m * l; // a camera adds nothing, not even a NaN, where its weight is zero
    a[c] = a[c] + t;
  }
  s = s + m;
  mb_store<C>(P.a, at, a);
  P.s[at] = s;
}

// ---------------------------------------------------------------- collapse: R_k = N_k + E(R_{k+1})
template <int C> __global__ __launch_bounds__(kMbThreads) void multiband_collapse_kernel(const MultibandCollapseParams P) {
  __shared__ float coarse[C][kMbExpandRows][kMbExpandCols];
  __shared__ float hor[C][kMbExpandRows][kMbTileW];
  static_assert(sizeof(coarse) + sizeof(hor) == (size_t)mb_expand_lds_bytes(C), "the LDS the design states");
  float e[C];
#pragma unroll
  for (int c = 0; c < C; ++c) e[c] = 0.0f;
  if (!P.top) mb_expand<C>(P.cr, P.cw, P.ch, P.wrap, coarse, hor, e); // (kernel-uniform)
  const int x = (int)blockIdx.x * kMbTileW + (int)threadIdx.x % kMbTileW;
  const int y = (int)blockIdx.y * kMbTileH + (int)threadIdx.x / kMbTileW;
  if (x >= P.w || y >= P.h) return;
  const size_t at = (size_t)y * (size_t)P.w + (size_t)x;
  float a[C], r[C];
  mb_load<C>(P.a, at, a);
  const float s = P.s[at];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float n = (s > 0.0f) ? a[c] / s : 0.0f;
    r[c] = P.top ? n : n + e[c];
  }
  if (P.label != nullptr) { // level 0
    if ((int)P.label[at] == kMultibandNoCamera) {
#pragma unroll
      for (int c = 0; c < C; ++c) r[c] = 0.0f;
    } else if (P.has_post) {
#pragma unroll
      for (int c = 0; c < (C < 3 ? C : 3); ++c) r[c] = tonemap(r[c], P.exposure, P.reinhard);
    }
  }
  mb_store<C>(P.dst, at, r);
}

} // namespace lrp
