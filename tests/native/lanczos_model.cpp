// lanczos_model.cpp — CPU model of the Lanczos-3 sampler (include/lrp.h "Lanczos-3"), test infrastructure: the definition
// restated from the header's text, independently of the kernels' lrp_lanczos.h (which this file must not include).  Only the
// sine and cosine come from the product (lrp_math.h: the clones that give the same bits on host and device).  Built by
// __graft_entry__.build() with -ffp-contract=off; bound by tests/lanczos_model.py.
#include <cstdint>
#include <cstddef>

#include "lrp_math.h"

namespace {

const float PI_F = 0x1.921fb6p+1f;
const float SIN60_F = 0x1.bb67aep-1f;

// int(float) of the reference's x86-64 build (cvttss2si): everything that does not fit, NaN included, is INT_MIN
int to_int(float v) {
  if (!(v > -2147483904.0f && v < 2147483648.0f)) return INT32_MIN;
  return (int)v;
}
int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// (i + W) % W in two's complement with C's remainder; a negative remainder reads column 0
int wrap_column(int i, int w) {
  const int t = (int)((uint32_t)i + (uint32_t)w);
  const int r = t % w;
  return r < 0 ? 0 : r;
}
int source_column(int i, int w, int loop) { return loop ? wrap_column(i, w) : clamp_int(i, 0, w - 1); }
// std::max(0.0f, std::min(1.0f, v)): min returns its first argument unless the second is smaller, max likewise
float clamp_unit(float v) {
  const float m = (v < 1.0f) ? v : 1.0f;
  return (0.0f < m) ? m : 0.0f;
}

struct Side {
  float near, mid, far; // distances t, t + 1, t + 2
};

Side side_weights(float t) {
  Side h;
  const float p = PI_F * t;
  const float s = lrp::sinf_(p);
  const float third = p / 3.0f;
  const float s3 = lrp::sinf_(third);
  const float c3 = lrp::cosf_(third);
  if (p == 0.0f) {
    h.near = 1.0f;
  } else {
    const float a = 3.0f * (s / p);
    const float b = s3 / p;
    h.near = a * b;
  }
  const float p1 = PI_F * (t + 1.0f);
  const float half_s3 = 0.5f * s3;
  const float k_c3 = SIN60_F * c3;
  const float a1 = half_s3 + k_c3;
  const float n1 = 3.0f * ((-s) * a1);
  h.mid = n1 / (p1 * p1);
  const float p2 = PI_F * (t + 2.0f);
  const float a2 = k_c3 - half_s3;
  const float n2 = 3.0f * (s * a2);
  h.far = n2 / (p2 * p2);
  return h;
}

void axis_weights(float f, float w[6]) {
  if (f == 0.0f || f == 1.0f) {
    for (int k = 0; k < 6; ++k) w[k] = 0.0f;
    w[f == 0.0f ? 2 : 3] = 1.0f;
    return;
  }
  const Side left = side_weights(f);
  const Side right = side_weights(1.0f - f);
  const float raw[6] = {left.far, left.mid, left.near, right.near, right.mid, right.far};
  float total = raw[0] + raw[1];
  total = total + raw[2];
  total = total + raw[3];
  total = total + raw[4];
  total = total + raw[5];
  for (int k = 0; k < 6; ++k) w[k] = raw[k] / total;
}

void sample(const float *src, int w, int h, int C, int loop, float sx, float sy, float *out) {
  int ix[6], iy[6];
  for (int k = -2; k <= 3; ++k) {
    ix[k + 2] = source_column(k == 0 ? to_int(sx) : to_int(sx + (float)k), w, loop);
    iy[k + 2] = clamp_int(k == 0 ? to_int(sy) : to_int(sy + (float)k), 0, h - 1);
  }
  const float fx = clamp_unit(sx - (float)ix[2]);
  const float fy = clamp_unit(sy - (float)iy[2]);
  float wx[6], wy[6];
  axis_weights(fx, wx);
  axis_weights(fy, wy);
  for (int c = 0; c < C; ++c) {
    float value = 0.0f;
    for (int i = 0; i < 6; ++i) {
      float col = wy[0] * src[((size_t)iy[0] * w + ix[i]) * C + c];
      for (int j = 1; j < 6; ++j) {
        const float term = wy[j] * src[((size_t)iy[j] * w + ix[i]) * C + c];
        col = col + term;
      }
      const float term = wx[i] * col;
      value = (i == 0) ? term : value + term;
    }
    out[c] = value;
  }
}

} // namespace

extern "C" {

void lzm_weights(float f, float *w) { axis_weights(f, w); }
// (the same for n fractions: w is (n, 6))
void lzm_weights_n(const float *f, long long n, float *w) {
  for (long long i = 0; i < n; ++i) axis_weights(f[i], w + 6 * i);
}

void lzm_sample(const float *src, int w, int h, int C, int loop, float sx, float sy, float *out) { sample(src, w, h, C, loop, sx, sy, out); }

// n_pixels output pixels of n2 sub-samples each; sxy: (n_pixels, n2, 2) in the loop's order (ssx outer, ssy inner);
// out: (n_pixels, C).  acc = 0; acc += sample per sub-sample; out = acc * normalize.  Returns 0, or 1 for C > 64.
int lzm_render(const float *src, int w, int h, int C, int loop, const float *sxy, long long n_pixels, int n2, float normalize, float *out) {
  if (C < 1 || C > 64) return 1;
  float acc[64], s[64];
  for (long long p = 0; p < n_pixels; ++p) {
    for (int c = 0; c < C; ++c) acc[c] = 0.0f;
    for (int k = 0; k < n2; ++k) {
      const float *xy = sxy + ((size_t)p * n2 + k) * 2;
      sample(src, w, h, C, loop, xy[0], xy[1], s);
      for (int c = 0; c < C; ++c) acc[c] += s[c];
    }
    for (int c = 0; c < C; ++c) out[(size_t)p * C + c] = acc[c] * normalize;
  }
  return 0;
}
}
