// lrp_mb_packed_kernel.h — the level-0 collapse of multi-band blending into a packed output (include/lrp.h "multi-band blending,
// packed pixels"), templated on the colour channel count C = 1 .. 4.  Included by lrp_mb_packed.hip alone.
//
// The bytes are those of multiband_collapse_kernel at level 0 -> lrp_encode_pixels_device.  Nothing is restated: the expand is
// mb_expand of lrp_multiband_kernel.h, the store is store_packed of lrp_packed_kernel.h (the 8-bit threshold search of the
// conversion kernels, the half conversion of include/lrp_half.h).
//
// Mapping (gfx950): that kernel's — 256 threads on a 32 x 8 tile of the output, one texel per lane, a plain 2-D grid; the coarse
// window 18 x 6 and the horizontal pass 32 x 6 in LDS, C x 1200 bytes, and behind them the 8-bit threshold table, 1 KiB, loaded
// by the 256 threads before any of them leaves (an 8-bit output only).  Byte offsets into the output are 32-bit.
#pragma once

#include <hip/hip_runtime.h>

#include "lrp_mb_packed.h"
#include "lrp_multiband_kernel.h"
#include "lrp_packed_kernel.h"

namespace lrp {

static_assert(kMbThreads == 256, "one thread per entry of the 8-bit threshold table");

template <int C> __global__ __launch_bounds__(kMbThreads) void mb_collapse_packed_kernel(const MbCollapsePackedParams P) {
  __shared__ float coarse[C][kMbExpandRows][kMbExpandCols];
  __shared__ float hor[C][kMbExpandRows][kMbTileW];
  __shared__ float thr[256];
  static_assert(sizeof(coarse) + sizeof(hor) + sizeof(thr) == (size_t)mb_collapse_packed_lds_bytes(C), "the LDS the design states");
  const bool want_thr = P.out_format == kPackedU8; // (kernel-uniform)
  if (want_thr) thr[threadIdx.x] = P.threshold[threadIdx.x];
  float e[C];
#pragma unroll
  for (int c = 0; c < C; ++c) e[c] = 0.0f;
  if (!P.top)
    mb_expand<C>(P.cr, P.cw, P.ch, P.wrap, coarse, hor, e); // (kernel-uniform; its barriers publish the table too)
  else if (want_thr)
    __syncthreads();
  const int x = (int)blockIdx.x * kMbTileW + (int)threadIdx.x % kMbTileW;
  const int y = (int)blockIdx.y * kMbTileH + (int)threadIdx.x / kMbTileW;
  if (x >= P.w || y >= P.h) return;
  const size_t at = (size_t)y * (size_t)P.w + (size_t)x;
  float a[C];
  mb_load<C>(P.a, at, a);
  const float s = P.s[at];
  Texel<4> r;
#pragma unroll
  for (int c = 0; c < 4; ++c) r.v[c] = 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float n = (s > 0.0f) ? a[c] / s : 0.0f;
    r.v[c] = P.top ? n : n + e[c];
  }
  if ((int)P.label[at] == kMultibandNoCamera) {
#pragma unroll
    for (int c = 0; c < C; ++c) r.v[c] = 0.0f;
  } else if (P.has_post) {
#pragma unroll
    for (int c = 0; c < (C < 3 ? C : 3); ++c) r.v[c] = tonemap(r.v[c], P.exposure, P.reinhard);
  }
  store_packed<4>(P, thr, (uint32_t)at, r);
}

} // namespace lrp
