// lrp_camview_kernel.h — the camera-view kernel (include/lrp.h "calibrated camera as the target"): frames
// of calibrated cameras composed into the frame of another calibrated camera — a new camera matrix, camera-to-camera remapping,
// re-distortion — with n x n sub-samples per pixel, one launch.  Included by one .hip unit per interpolation (lrp_camview.hip,
// lrp_camview_bl.hip, lrp_camview_bc.hip) so that the three instantiation sets compile in parallel.
//
// Per output pixel: compose_cam_kernel (lrp_camera_kernel.h) with one thing replaced: target_ray<OutLens> of an ideal lens by
// camera_unproject<TargetModel> (lrp_camera_inverse.h), the Newton inverse of the target's polynomial, which may find no ray.
// A sub-sample without a ray is covered by no camera.  camera_project, sample<> and compose_min are restated nowhere.
//
// Mapping (gfx950): compose_cam_kernel's — the 32 x 8 tile, one pixel per lane, tiles in xcd_tile() order, Texel<0> run-time
// channels, wave-uniform loops that are not unrolled (the Newton loop among them), descriptors in SGPRs, a wave-wide ballot per
// source and sub-sample, the FIRST early exit; and a ballot after the inverse, so that a wave none of whose lanes has a ray
// skips the source loop.  The target's model is a template parameter (one target per launch): 2 models x 3 samplers.  The
// sources' models stay a wave-uniform branch.  No LDS.
#pragma once

#include "lrp_camera_inverse.h"
#include "lrp_camera_kernel.h"
#include "lrp_camview.h"

namespace lrp {

using CameraViewKernelFn = void (*)(const CameraViewParams);

template <int TargetModel, int Interp>
__global__ __launch_bounds__(kComposeThreads) void camera_view_kernel(const CameraViewParams P) {
  constexpr int L = texel_lanes<0>();
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;

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
    const float u = ((float)x + ((float)ssx + 1.0f) / ns1) - 0.5f; // pixels of the target; n == 1: u == x
#pragma unroll 1
    for (int ssy = 0; ssy < ns; ++ssy) {
      const float v0 = ((float)y + ((float)ssy + 1.0f) / ns1) - 0.5f;
      float rx, ry, rz; // the target ray, once for all cameras
      const bool has_ray = camera_unproject<TargetModel>(P.target, u, v0, rx, ry, rz);
      if (__builtin_amdgcn_ballot_w64(has_ray) == 0ull) continue; // no lane of the wave has a ray: no camera is asked

      // ---- the body of compose_cam_kernel for this sub-sample: v_j, k_j
      Texel<0> v;
#pragma unroll
      for (int c = 0; c < L; ++c) v.v[c] = 0.0f;
      float wsum = 0.0f;
      uint32_t k = 0;
#pragma unroll 1
      for (int i = 0; i < P.n_src; ++i) {
        const CameraSource &S = P.src[i]; // wave-uniform
        float vx = rx, vy = ry, vz = rz;
        if (S.has_rot) {
          vx = S.rot[0] * rx + S.rot[1] * ry + S.rot[2] * rz;
          vy = S.rot[3] * rx + S.rot[4] * ry + S.rot[5] * rz;
          vz = S.rot[6] * rx + S.rot[7] * ry + S.rot[8] * rz;
        }
        const float in_w = (float)S.in_w, in_h = (float)S.in_h;
        float sx, sy;
        const bool imaged = camera_project(S, vx, vy, vz, sx, sy);
        // covered iff has_ray && imaged && in_x && in_y; comparisons with NaN are false
        const bool covered = has_ray && imaged && sx >= -0.5f && sx <= in_w - 0.5f && sy >= -0.5f && sy <= in_h - 0.5f;
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
        // FIRST: every lane that has a ray has its value (a count plane wants to see all cameras)
        if (mode == kComposeFirst && P.count == nullptr && __builtin_amdgcn_ballot_w64(has_ray && k == 0u) == 0ull) break;
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
    if (P.has_post) { // fused post_process: the first min(C, 3) channels
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

template <int Interp> hipError_t launch_camera_view_interp(CameraViewParams P, hipStream_t stream) {
  P.tiles_x = (P.out_w + kComposeTileW - 1) / kComposeTileW;
  P.tiles_y = (P.out_h + kComposeTileH - 1) / kComposeTileH;
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  CameraViewKernelFn fn = nullptr;
  if (P.target.model == kCameraBrown) fn = camera_view_kernel<kCameraBrown, Interp>;
  if (P.target.model == kCameraFisheye) fn = camera_view_kernel<kCameraFisheye, Interp>;
  if (!fn) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
