// lrp_lanczos.h — the Lanczos-3 sampler (include/lrp.h "Lanczos-3"): a 6 x 6 footprint, weights
// sinc(d) sinc(d / 3) normalised per axis.  An opt-in extension (lrp_sampler_extensions); the reference has no such sampler,
// so the definition of include/lrp.h is the yardstick and tests/native/lanczos_model.cpp restates it on the CPU.
//
// All arithmetic is binary32, un-fused, in the order include/lrp.h writes it (the units are compiled with
// -ffp-contract=off); sinf_ / cosf_ are the clones of lrp_math.h, the index rules are those of sample_bicubic.
#pragma once

#include "lrp_device.h"

namespace lrp {

constexpr float kLzPi = 0x1.921fb6p+1f;
constexpr float kLzSin60 = 0x1.bb67aep-1f;
constexpr int kLzTaps = 6; // k = -2 .. 3

// The weights of the taps at distances t, t + 1, t + 2 (0 < t <= 1) on one side of the sample position, not normalised.
// sin(pi (t + j)) = +-sin(pi t), and sin(pi (t + j) / 3) from the angle sum with sin(pi t / 3), cos(pi t / 3): two
// trigonometric calls for three taps.
__device__ __forceinline__ void lanczos_half(float t, float &h0, float &h1, float &h2) {
  const float p = kLzPi * t;
  const float s = sinf_(p);
  const float q = p / 3.0f;
  const float s3 = sinf_(q);
  const float c3 = cosf_(q);
  h0 = (p == 0.0f) ? 1.0f : (3.0f * (s / p)) * (s3 / p);
  const float p1 = kLzPi * (t + 1.0f);
  const float a1 = (0.5f * s3) + (kLzSin60 * c3);
  h1 = (3.0f * ((-s) * a1)) / (p1 * p1);
  const float p2 = kLzPi * (t + 2.0f);
  const float a2 = (kLzSin60 * c3) - (0.5f * s3);
  h2 = (3.0f * (s * a2)) / (p2 * p2);
}

// The six weights of one axis from the fraction f in [0, 1], tap order k = -2 .. 3.  The right-hand taps are evaluated at
// 1 - f, so the weight next to the nearest tap keeps its relative accuracy on both sides.
__device__ __forceinline__ void lanczos_axis(float f, float w[kLzTaps]) {
  if (f == 0.0f || f == 1.0f) {
#pragma unroll
    for (int k = 0; k < kLzTaps; ++k) w[k] = 0.0f;
    if (f == 0.0f)
      w[2] = 1.0f;
    else
      w[3] = 1.0f;
    return;
  }
  float r[kLzTaps];
  lanczos_half(f, r[2], r[1], r[0]);
  lanczos_half(1.0f - f, r[3], r[4], r[5]);
  const float W = ((((r[0] + r[1]) + r[2]) + r[3]) + r[4]) + r[5];
#pragma unroll
  for (int k = 0; k < kLzTaps; ++k) w[k] = r[k] / W;
}

// The blend: vertical per tap column, then horizontal, like bicubicInterpolate; every step is a multiply, then an add.
// tap(i, j) -> Texel<CH>: the texel of tap column i, tap row j (0 .. 5).  The horizontal sum is carried along as the
// columns complete: the same operations in the same order as summing the six finished columns.
template <int CH, class Tap>
__device__ __forceinline__ Texel<CH> lanczos_blend(const float wx[kLzTaps], const float wy[kLzTaps], const Tap tap) {
  constexpr int L = texel_lanes<CH>();
  Texel<CH> r;
#pragma unroll
  for (int i = 0; i < kLzTaps; ++i) {
    Texel<CH> col;
#pragma unroll
    for (int j = 0; j < kLzTaps; ++j) {
      const Texel<CH> p = tap(i, j);
#pragma unroll
      for (int c = 0; c < L; ++c) {
        const float m = wy[j] * p.v[c];
        col.v[c] = j == 0 ? m : col.v[c] + m;
      }
    }
#pragma unroll
    for (int c = 0; c < L; ++c) {
      const float m = wx[i] * col.v[c];
      r.v[c] = i == 0 ? m : r.v[c] + m;
    }
  }
  return r;
}

// The fractions of a sample position: from the CLAMPED index of tap k = 0, as the reference's bicubic takes them.
template <bool Loop> __device__ __forceinline__ void lanczos_fractions(const KParams &P, float sx, float sy, float &fx, float &fy) {
  const int ix0 = column<Loop>(trunc_x86(sx), P.in_w);
  const int iy0 = clamp_index(trunc_x86(sy), P.in_h - 1);
  fx = unit_clamp(sx - (float)ix0);
  fy = unit_clamp(sy - (float)iy0);
}

// The sampler with its 36 taps gathered from the source image.
template <int CH, bool Loop> __device__ __forceinline__ Texel<CH> sample_lanczos(const KParams &P, float sx, float sy) {
  const int w = P.in_w, h = P.in_h;
  const uint32_t C = (uint32_t)P.channels;
  uint32_t xs[kLzTaps], rows[kLzTaps];
#pragma unroll
  for (int k = 0; k < kLzTaps; ++k) {
    const float d = (float)(k - 2);
    xs[k] = (uint32_t)column<Loop>(k == 2 ? trunc_x86(sx) : trunc_x86(sx + d), w);
    rows[k] = (uint32_t)clamp_index(k == 2 ? trunc_x86(sy) : trunc_x86(sy + d), h - 1) * (uint32_t)w;
  }
  float fx, fy;
  lanczos_fractions<Loop>(P, sx, sy, fx, fy);
  float wx[kLzTaps], wy[kLzTaps];
  lanczos_axis(fx, wx);
  lanczos_axis(fy, wy);
  return lanczos_blend<CH>(wx, wy, [&](int i, int j) { return load_texel<CH>(P.src, (rows[j] + xs[i]) * C, P.ch_count); });
}

} // namespace lrp
