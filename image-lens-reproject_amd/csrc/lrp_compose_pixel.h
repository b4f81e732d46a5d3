// lrp_compose_pixel.h — the per-pixel body of the supersampled compose kernels: what one lane does from
// the bounds check of its pixel to its three stores, written once for compose_ss_kernel, compose_cam_kernel, camgain_kernel and
// camera_view_kernel (lrp_compose_ss_kernel.h, lrp_camera_kernel.h, lrp_camgain_kernel.h, lrp_camview_kernel.h).
//
// Per sub-sample: the target ray once; then, source by source, the rotation, the source mapping with its coverage test
// (include/lrp.h "coverage"), a sample<> of the sources that cover it, composed under `mode` (FIRST, MEAN, FEATHER) — the body
// of compose_kernel (lrp_compose_kernel.h) inside the two sub-sample loops of lrp_kernel_impl.h.  What the kernels differ in:
//
//   Sources  static bool map(S, vx, vy, vz, in_w, in_h, sx, sy): the rotated ray to source pixel coordinates, returns
//            `covered`; constexpr bool kLoop: the sampler wraps in x.  LensSources<InMode> (lrp_compose_kernel.h),
//            CameraSources (lrp_camera_kernel.h).
//   Target   the per-pixel state of the output side, built from (P, x, y); column(ssx, ns1): the coordinate of sub-sample
//            column ssx; ray(P, column, ssy, ns1, rx, ry, rz): the ray of sub-sample (ssx, ssy), returns has_ray; constexpr
//            bool kAlwaysRay: has_ray is true by construction, and the tests of it are not compiled.  IdealTarget<OutLens>
//            below, CameraTarget<Model> (lrp_camview_kernel.h).
//   hook     hook(i), at the head of the source loop, gives what is applied to the sample of source i right after it is
//            taken: on_sample(s, ch_count).  NoSampleHook below, CameraGainHook (lrp_camgain_kernel.h).
//
// The body is ONE __forceinline__ function and takes the kernel's argument block by const reference: by value the block is
// copied to scratch, and with the source loop as a function of its own registers move (DESIGN.md section 20 has the figures).
// The arithmetic is in the order of src/reproject.cpp; the bytes depend on it.
//
// Mapping (gfx950): compose's — the 32 x 8 tile, one pixel per lane, tiles in xcd_tile() order, Texel<0> run-time channels,
// the source descriptors in SGPRs (scalar loads from the kernarg block), a wave-wide ballot per source and sub-sample so that
// a source no lane's sub-sample needs forms no address, the FIRST early exit.  All three loops are wave-uniform (n and n_src
// are kernarg values) and not unrolled: one instantiation set serves every n.  A lane's sub-samples lie within a texel or two
// of each other, so its gathers hit the lines it has just loaded.  State that lives across sub-samples: the accumulator, m and
// an 8-bit mask of the sources seen (the count plane is its popcount).  No LDS.
#pragma once

#include "lrp_compose_kernel.h"

namespace lrp {

// The target of an ideal lens: the sub-sample positions of src/reproject.cpp:287-298 and target_ray<OutLens>.
template <int OutLens> struct IdealTarget {
  static constexpr bool kAlwaysRay = true;
  float cx, cy; // pixel centre in image-centred coordinates (src/reproject.cpp:287-288)
  template <typename Params>
  __device__ __forceinline__ IdealTarget(const Params &P, int x, int y)
      : cx(((float)x + 0.5f) - (float)P.out_w * 0.5f), cy(((float)y + 0.5f) - (float)P.out_h * 0.5f) {}
  __device__ __forceinline__ float column(int ssx, float ns1) const { return cx + ((float)ssx + 1.0f) / ns1 - 0.5f; } // :295
  template <typename Params>
  __device__ __forceinline__ bool ray(const Params &P, float scx, int ssy, float ns1, float &rx, float &ry, float &rz) const {
    const float scy = cy + ((float)ssy + 1.0f) / ns1 - 0.5f; // :298
    target_ray<OutLens>(P.out_lens, (float)P.out_w, (float)P.out_h, scx, scy, rx, ry, rz);
    return true;
  }
};

// The hook of a kernel that leaves the samples as they are.
struct NoSampleHook {
  struct Apply {
    __device__ __forceinline__ void operator()(Texel<0> &, int) const {}
  };
  __device__ __forceinline__ Apply operator()(int) const { return {}; }
};

// Pixel (x, y), which lies inside the output: its n x n sub-samples to its three stores.  Per sub-sample j the sources are
// composed under `mode` into v_j; the covered sub-samples' v_j are summed in ascending j (ssx outside, ssy inside) and divided
// by their number m.
template <int Interp, typename Sources, typename Target, typename Params, typename Hook>
__device__ __forceinline__ void compose_ss_pixel(const Params &P, int x, int y, const Hook &hook) {
  constexpr int L = texel_lanes<0>();
  const Target T(P, x, y);
  const int mode = P.mode;
  const int ns = P.num_samples;
  const float ns1 = (float)ns + 1.0f;
  Texel<0> acc; // the sum of v_j over the covered sub-samples
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  uint32_t m = 0;    // covered sub-samples
  uint32_t seen = 0; // bit i: source i covers at least one sub-sample

#pragma unroll 1
  for (int ssx = 0; ssx < ns; ++ssx) {
    const float col = T.column(ssx, ns1);
#pragma unroll 1
    for (int ssy = 0; ssy < ns; ++ssy) {
      float rx, ry, rz; // the target ray, once for all sources
      const bool has_ray = T.ray(P, col, ssy, ns1, rx, ry, rz);
      if constexpr (!Target::kAlwaysRay)
        if (__builtin_amdgcn_ballot_w64(has_ray) == 0ull) continue; // no lane of the wave has a ray: no source is asked

      // ---- v_j, k_j of this sub-sample
      Texel<0> v;
#pragma unroll
      for (int c = 0; c < L; ++c) v.v[c] = 0.0f;
      float wsum = 0.0f;
      uint32_t k = 0;
#pragma unroll 1
      for (int i = 0; i < P.n_src; ++i) {
        const auto &S = P.src[i]; // wave-uniform
        const auto on_sample = hook(i); // wave-uniform
        float vx = rx, vy = ry, vz = rz;
        if (S.has_rot) { // src/reproject.cpp:301-311
          vx = S.rot[0] * rx + S.rot[1] * ry + S.rot[2] * rz;
          vy = S.rot[3] * rx + S.rot[4] * ry + S.rot[5] * rz;
          vz = S.rot[6] * rx + S.rot[7] * ry + S.rot[8] * rz;
        }
        const float in_w = (float)S.in_w, in_h = (float)S.in_h;
        float sx, sy;
        bool covered = Sources::map(S, vx, vy, vz, in_w, in_h, sx, sy);
        if constexpr (!Target::kAlwaysRay) covered = has_ray && covered; // a sub-sample without a ray is covered by no source
        const bool need = covered && (mode != kComposeFirst || k == 0u);
        if (__builtin_amdgcn_ballot_w64(need) != 0ull) { // a source no lane's sub-sample needs is not sampled
          if (need) {
            KParams Q; // the sampler's view of source i: sample<> reads these five fields of a KParams and nothing else
            Q.src = S.data;
            Q.in_w = S.in_w;
            Q.in_h = S.in_h;
            Q.channels = P.channels;
            Q.ch_count = P.ch_count;
            Texel<0> s = sample<Interp, 0, Sources::kLoop>(Q, sx, sy);
            on_sample(s, P.ch_count);
            if (mode == kComposeFeather) {
              const float dy = compose_min(sy + 0.5f, (in_h - 0.5f) - sy);
              float d = dy;
              if constexpr (!Sources::kLoop) d = compose_min(compose_min(sx + 0.5f, (in_w - 0.5f) - sx), dy);
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
        // FIRST: every lane that has a ray has its value (a count plane wants to see all sources)
        bool waiting = k == 0u;
        if constexpr (!Target::kAlwaysRay) waiting = has_ray && waiting;
        if (mode == kComposeFirst && P.count == nullptr && __builtin_amdgcn_ballot_w64(waiting) == 0ull) break;
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

} // namespace lrp
