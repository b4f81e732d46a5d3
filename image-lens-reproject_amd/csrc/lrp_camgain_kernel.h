// lrp_camgain_kernel.h — the calibrated-camera compose kernel with one gain per camera (include/lrp.h "exposure matching across
// a camera rig").  Included by one .hip unit per interpolation (lrp_camgain.hip, lrp_camgain_bl.hip,
// lrp_camgain_bc.hip) so that the three instantiation sets compile in parallel.
//
// Per output pixel: compose_cam_kernel (lrp_camera_kernel.h) with one insertion: right after sampling, the first min(C, 3)
// channels of s_i are multiplied by g_i — one v_mul_f32 per channel, ahead of the FIRST / MEAN / FEATHER arithmetic.  A kernel
// of its own, so that compose_cam_kernel's code object does not move; camera_project, target_ray, sample<> and compose_min are
// restated nowhere.  This kernel is launched for the first group of 8 channels only: the later groups hold no channel below 3
// and go through compose_cam_kernel itself.
//
// Mapping (gfx950): compose_cam_kernel's, unchanged; g_i is one more scalar load from the kernarg block.  No LDS.
#pragma once

#include "lrp_camera_kernel.h"
#include "lrp_camgain.h"

namespace lrp {

using CameraGainKernelFn = void (*)(const CameraGainParams);

template <int OutLens, int Interp>
__global__ __launch_bounds__(kComposeThreads) void camgain_kernel(const CameraGainParams G) {
  constexpr int L = texel_lanes<0>();
  const CameraParams &P = G.cam;
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;

  const float cx = ((float)x + 0.5f) - (float)P.out_w * 0.5f;
  const float cy = ((float)y + 0.5f) - (float)P.out_h * 0.5f;

  const int mode = P.mode;
  const int ns = P.num_samples;
  const float ns1 = (float)ns + 1.0f;
  Texel<0> acc; // the sum of v_j over the covered sub-samples
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  uint32_t m = 0;    // covered sub-samples
  uint32_t seen = 0; // bit i: camera i covers at least one sub-sample

#pragma unroll 1
  for (int ssx = 0; ssx < ns; ++ssx) {
    const float scx = cx + ((float)ssx + 1.0f) / ns1 - 0.5f;
#pragma unroll 1
    for (int ssy = 0; ssy < ns; ++ssy) {
      const float scy = cy + ((float)ssy + 1.0f) / ns1 - 0.5f;
      float rx, ry, rz; // the target ray, once for all cameras
      target_ray<OutLens>(P.out_lens, (float)P.out_w, (float)P.out_h, scx, scy, rx, ry, rz);

      Texel<0> v;
#pragma unroll
      for (int c = 0; c < L; ++c) v.v[c] = 0.0f;
      float wsum = 0.0f;
      uint32_t k = 0;
#pragma unroll 1
      for (int i = 0; i < P.n_src; ++i) {
        const CameraSource &S = P.src[i]; // wave-uniform
        const float gain = G.gain[i];     // wave-uniform
        float vx = rx, vy = ry, vz = rz;
        if (S.has_rot) {
          vx = S.rot[0] * rx + S.rot[1] * ry + S.rot[2] * rz;
          vy = S.rot[3] * rx + S.rot[4] * ry + S.rot[5] * rz;
          vz = S.rot[6] * rx + S.rot[7] * ry + S.rot[8] * rz;
        }
        const float in_w = (float)S.in_w, in_h = (float)S.in_h;
        float sx, sy;
        const bool imaged = camera_project(S, vx, vy, vz, sx, sy);
        const bool covered = imaged && sx >= -0.5f && sx <= in_w - 0.5f && sy >= -0.5f && sy <= in_h - 0.5f;
        const bool need = covered && (mode != kComposeFirst || k == 0u);
        if (__builtin_amdgcn_ballot_w64(need) != 0ull) { // a camera no lane's sub-sample needs is not sampled
          if (need) {
            KParams Q; // the sampler's view of camera i
            Q.src = S.data;
            Q.in_w = S.in_w;
            Q.in_h = S.in_h;
            Q.channels = P.channels;
            Q.ch_count = P.ch_count;
            Texel<0> s = sample<Interp, 0, false>(Q, sx, sy);
#pragma unroll
            for (int c = 0; c < 3; ++c) // the gain: colour only (this launch's channel 0 is the image's)
              if (c < P.ch_count) s.v[c] = gain * s.v[c];
            if (mode == kComposeFeather) {
              const float dy = compose_min(sy + 0.5f, (in_h - 0.5f) - sy);
              const float d = compose_min(compose_min(sx + 0.5f, (in_w - 0.5f) - sx), dy);
              const float w = (d < 0x1p-10f) ? 0x1p-10f : d;
#pragma unroll
              for (int c = 0; c < L; ++c) {
                const float t = w * s.v[c];
                v.v[c] = v.v[c] + t;
              }
              wsum = wsum + w;
            } else if (mode == kComposeMean) {
#pragma unroll
              for (int c = 0; c < L; ++c) v.v[c] = v.v[c] + s.v[c];
            } else {
#pragma unroll
              for (int c = 0; c < L; ++c) v.v[c] = s.v[c];
            }
          }
        }
        k += covered ? 1u : 0u;
        seen |= covered ? (1u << i) : 0u;
        // FIRST: every lane has its value (a count plane wants to see all cameras)
        if (mode == kComposeFirst && P.count == nullptr && __builtin_amdgcn_ballot_w64(k == 0u) == 0ull) break;
      }

      if (k != 0u) { // an uncovered sub-sample adds nothing and is not counted
        if (mode != kComposeFirst) {
          const float div = mode == kComposeMean ? (float)k : wsum;
#pragma unroll
          for (int c = 0; c < L; ++c) v.v[c] = v.v[c] / div;
        }
#pragma unroll
        for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] + v.v[c];
        m += 1u;
      }
    }
  }

  if (m == 0u) { // no sub-sample is covered: +0.0f in every channel, whatever post is
#pragma unroll
    for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  } else {
    const float r = 1.0f / (float)m;
#pragma unroll
    for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] * r;
    if (P.has_post) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c < P.ch_count) acc.v[c] = tonemap(acc.v[c], P.exposure, P.reinhard);
    }
  }
  const uint32_t px_index = (uint32_t)y * (uint32_t)P.out_w + (uint32_t)x;
  store_texel<0>(P.dst, px_index * (uint32_t)P.channels, acc, P.ch_count);
  if (P.count != nullptr) P.count[px_index] = (uint8_t)__builtin_popcount(seen);
  if (P.coverage != nullptr) P.coverage[px_index] = (uint8_t)m;
}

// The kernels: one per output lens id.
template <int Interp, int... OutLens>
constexpr std::array<CameraGainKernelFn, kLensIds> camgain_kernel_table(std::integer_sequence<int, OutLens...>) {
  return {{camgain_kernel<OutLens, Interp>...}};
}
template <int Interp> CameraGainKernelFn camgain_kernel_of(int out_lens) {
  static constexpr std::array<CameraGainKernelFn, kLensIds> table = camgain_kernel_table<Interp>(std::make_integer_sequence<int, kLensIds>{});
  if (out_lens < 0 || out_lens >= kLensIds) return nullptr;
  return table[out_lens];
}

template <int Interp> hipError_t launch_compose_cameras_gain_interp(CameraGainParams G, int out_lens, hipStream_t stream) {
  CameraParams &P = G.cam;
  P.tiles_x = (P.out_w + kComposeTileW - 1) / kComposeTileW;
  P.tiles_y = (P.out_h + kComposeTileH - 1) / kComposeTileH;
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  const CameraGainKernelFn fn = camgain_kernel_of<Interp>(out_lens);
  if (!fn) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, G);
  return hipGetLastError();
}

} // namespace lrp
