// lrp_camera_kernel.h — the calibrated-camera compose kernel (include/lrp.h "compose, calibrated cameras", DESIGN.md section
// 17): several frames of calibrated cameras — fx, fy, cx, cy in pixels plus Brown-Conrady or Kannala-Brandt coefficients —
// into one output with n x n sub-samples per pixel, one launch.  Included by one .hip unit per interpolation (lrp_camera.hip,
// lrp_camera_bl.hip, lrp_camera_bc.hip) so that the three instantiation sets compile in parallel.
//
// Per output pixel: compose_ss_kernel (lrp_compose_ss_kernel.h) with one thing replaced: ray_to_source and the coverage test
// of an ideal lens by camera_project below, the closed-form polynomial from ray to source pixel and its `imaged` test.  No
// target lens and no sampler is restated: target_ray and sample<> are lrp_device.h's, compose_min lrp_compose_kernel.h's,
// atan2f_ lrp_math.h's.
//
// Mapping (gfx950): compose_ss_kernel's — the 32 x 8 tile, one pixel per lane, tiles in xcd_tile() order, Texel<0> run-time
// channels, three wave-uniform loops that are not unrolled, the camera descriptors in SGPRs (scalar loads from the kernarg
// block: nine rotation floats and twelve camera floats per source, none of which occupies a VGPR across the loop), a
// wave-wide ballot per source and sub-sample so that a camera no lane's sub-sample needs forms no address, the FIRST early
// exit.  The camera model is a wave-uniform branch on an SGPR, not a template parameter: rigs may mix models, and the
// instantiations stay at 5 output lenses x 3 samplers.  No LDS.
#pragma once

#include "lrp_camera.h"
#include "lrp_compose_kernel.h"

namespace lrp {

using CameraKernelFn = void (*)(const CameraParams);

// Ray -> source pixel of camera S (include/lrp.h "compose, calibrated cameras"): binary32, un-fused, in the order written
// there.  Returns `imaged`.
__device__ __forceinline__ bool camera_project(const CameraSource &S, float vx, float vy, float vz, float &sx, float &sy) {
  if (S.model == kCameraFisheye) { // wave-uniform
    const float rho = lrp_sqrtf(vx * vx + vy * vy);
    const float theta = atan2f_(rho, -vz);
    const float t2 = theta * theta;
    const float td = theta * (1.0f + t2 * (S.k[0] + t2 * (S.k[1] + t2 * (S.k[2] + t2 * S.k[3]))));
    const float q = (rho > 0.0f) ? td / rho : 0.0f;
    sx = S.fx * (q * vx) + S.cx;
    sy = S.fy * (q * vy) + S.cy;
    return theta <= S.limit;
  }
  const float k1 = S.k[0], k2 = S.k[1], p1 = S.k[2], p2 = S.k[3], k3 = S.k[4];
  const float a = vx / -vz;
  const float b = vy / -vz;
  const float r2 = a * a + b * b;
  const float ab = a * b;
  const float L = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
  const float xd = a * L + ((2.0f * p1) * ab + p2 * (r2 + 2.0f * (a * a)));
  const float yd = b * L + (p1 * (r2 + 2.0f * (b * b)) + (2.0f * p2) * ab);
  sx = S.fx * xd + S.cx;
  sy = S.fy * yd + S.cy;
  return vz < 0.0f && r2 <= S.limit;
}

template <int OutLens, int Interp>
__global__ __launch_bounds__(kComposeThreads) void compose_cam_kernel(const CameraParams P) {
  constexpr int L = texel_lanes<0>();
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;

  // pixel centre in image-centred coordinates (src/reproject.cpp:287-288)
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
    const float scx = cx + ((float)ssx + 1.0f) / ns1 - 0.5f; // src/reproject.cpp:295
#pragma unroll 1
    for (int ssy = 0; ssy < ns; ++ssy) {
      const float scy = cy + ((float)ssy + 1.0f) / ns1 - 0.5f; // src/reproject.cpp:298
      float rx, ry, rz; // the target ray, once for all cameras
      target_ray<OutLens>(P.out_lens, (float)P.out_w, (float)P.out_h, scx, scy, rx, ry, rz);

      // ---- the body of compose_kernel for this sub-sample: v_j, k_j
      Texel<0> v;
#pragma unroll
      for (int c = 0; c < L; ++c) v.v[c] = 0.0f;
      float wsum = 0.0f;
      uint32_t k = 0;
#pragma unroll 1
      for (int i = 0; i < P.n_src; ++i) {
        const CameraSource &S = P.src[i]; // wave-uniform
        float vx = rx, vy = ry, vz = rz;
        if (S.has_rot) { // src/reproject.cpp:301-311
          vx = S.rot[0] * rx + S.rot[1] * ry + S.rot[2] * rz;
          vy = S.rot[3] * rx + S.rot[4] * ry + S.rot[5] * rz;
          vz = S.rot[6] * rx + S.rot[7] * ry + S.rot[8] * rz;
        }
        const float in_w = (float)S.in_w, in_h = (float)S.in_h;
        float sx, sy;
        const bool imaged = camera_project(S, vx, vy, vz, sx, sy);
        // covered iff imaged && in_x && in_y; comparisons with NaN are false
        const bool covered = imaged && sx >= -0.5f && sx <= in_w - 0.5f && sy >= -0.5f && sy <= in_h - 0.5f;
        const bool need = covered && (mode != kComposeFirst || k == 0u);
        if (__builtin_amdgcn_ballot_w64(need) != 0ull) { // a camera no lane's sub-sample needs is not sampled
          if (need) {
            KParams Q; // the sampler's view of camera i: sample<> reads these five fields of a KParams and nothing else
            Q.src = S.data;
            Q.in_w = S.in_w;
            Q.in_h = S.in_h;
            Q.channels = P.channels;
            Q.ch_count = P.ch_count;
            const Texel<0> s = sample<Interp, 0, false>(Q, sx, sy);
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
    const float r = 1.0f / (float)m; // m == n * n: the reference's normalize (src/reproject.cpp:280)
#pragma unroll
    for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] * r;
    if (P.has_post) { // fused post_process: the first min(C, 3) channels (src/reproject.cpp:423-434)
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

// The kernels: one per output lens id (0 .. kLensIds - 1; the extension lenses are gated by the caller's validation).
template <int Interp, int... OutLens>
constexpr std::array<CameraKernelFn, kLensIds> camera_kernel_table(std::integer_sequence<int, OutLens...>) {
  return {{compose_cam_kernel<OutLens, Interp>...}};
}
// The kernel of output lens out_lens; nullptr: no such lens.
template <int Interp> CameraKernelFn camera_kernel(int out_lens) {
  static_assert(is_lens_id(0) && is_lens_id(kLensIds - 1), "every id 0 .. kLensIds - 1 names a lens");
  static constexpr std::array<CameraKernelFn, kLensIds> table = camera_kernel_table<Interp>(std::make_integer_sequence<int, kLensIds>{});
  if (out_lens < 0 || out_lens >= kLensIds) return nullptr;
  return table[out_lens];
}

template <int Interp> hipError_t launch_compose_cameras_interp(CameraParams P, int out_lens, hipStream_t stream) {
  P.tiles_x = (P.out_w + kComposeTileW - 1) / kComposeTileW;
  P.tiles_y = (P.out_h + kComposeTileH - 1) / kComposeTileH;
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  const CameraKernelFn fn = camera_kernel<Interp>(out_lens);
  if (!fn) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
