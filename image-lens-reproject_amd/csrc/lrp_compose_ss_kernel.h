// lrp_compose_ss_kernel.h — the supersampled compose kernel (include/lrp.h "compose, supersampled"):
// several source images into one output with n x n sub-samples per pixel, one launch.  Included by one .hip unit per
// interpolation (lrp_compose_ss.hip, lrp_compose_ss_bl.hip, lrp_compose_ss_bc.hip) so that the three instantiation sets
// compile in parallel.
//
// Per output pixel: the two sub-sample loops of lrp_kernel_impl.h (ssx outside, ssy inside, the positions of
// src/reproject.cpp:295,298) around the body of compose_kernel (lrp_compose_kernel.h): per sub-sample the target ray once,
// then, source by source, the rotation, ray_to_source, the coverage test and a sample<> of the sources that cover it,
// composed under `mode` into v_j; the covered sub-samples' v_j are summed in ascending j and divided by their number m.
// No lens formula, sampler or coverage test is restated: target_ray, ray_to_source and sample<> are lrp_device.h's,
// compose_covered and compose_min are lrp_compose_kernel.h's.
//
// Mapping (gfx950): compose's — the 32 x 8 tile, one pixel per lane, tiles in xcd_tile() order, Texel<0> run-time channels,
// the source descriptors in SGPRs (scalar loads from the kernarg block), a wave-wide ballot per source and sub-sample so
// that a source no lane's sub-sample needs forms no address.  All three loops are wave-uniform (n and n_src are kernarg
// values) and not unrolled: one instantiation set serves every n.  A lane's sub-samples lie within a texel or two of each
// other, so its gathers hit the lines it has just loaded.  State that lives across sub-samples: the accumulator, m and an
// 8-bit mask of the sources seen (the count plane is its popcount).  No LDS.
#pragma once

#include "lrp_compose_kernel.h"
#include "lrp_compose_ss.h"

namespace lrp {

using ComposeSsKernelFn = void (*)(const ComposeSsParams);

template <int OutLens, int InMode, int Interp>
__global__ __launch_bounds__(kComposeThreads) void compose_ss_kernel(const ComposeSsParams P) {
  constexpr bool Loop = (InMode == kInEquirectLoop);
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
  uint32_t seen = 0; // bit i: source i covers at least one sub-sample

#pragma unroll 1
  for (int ssx = 0; ssx < ns; ++ssx) {
    const float scx = cx + ((float)ssx + 1.0f) / ns1 - 0.5f; // src/reproject.cpp:295
#pragma unroll 1
    for (int ssy = 0; ssy < ns; ++ssy) {
      const float scy = cy + ((float)ssy + 1.0f) / ns1 - 0.5f; // src/reproject.cpp:298
      float rx, ry, rz; // the target ray, once for all sources
      target_ray<OutLens>(P.out_lens, (float)P.out_w, (float)P.out_h, scx, scy, rx, ry, rz);

      // ---- the body of compose_kernel for this sub-sample: v_j, k_j
      Texel<0> v;
#pragma unroll
      for (int c = 0; c < L; ++c) v.v[c] = 0.0f;
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
        if (__builtin_amdgcn_ballot_w64(need) != 0ull) { // a source no lane's sub-sample needs is not sampled
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
              float d = dy;
              if constexpr (!Loop) d = compose_min(compose_min(sx + 0.5f, (in_w - 0.5f) - sx), dy);
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
        // FIRST: every lane has its value (a count plane wants to see all sources)
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

// The cells: all 30, per interpolation, in the layout of compose_cell_table (entry out_lens * kInModes + in_mode).
template <int Interp, int Cell> constexpr ComposeSsKernelFn compose_ss_cell_entry() {
  if constexpr (is_lens_id(Cell / kInModes))
    return compose_ss_kernel<Cell / kInModes, Cell % kInModes, Interp>;
  else
    return nullptr;
}
template <int Interp, int... Cell>
constexpr std::array<ComposeSsKernelFn, kLensIds * kInModes> compose_ss_cell_table(std::integer_sequence<int, Cell...>) {
  return {{compose_ss_cell_entry<Interp, Cell>()...}};
}
// The kernel of cell (out_lens, in_mode); nullptr: no such cell.
template <int Interp> ComposeSsKernelFn compose_ss_cell_kernel(int out_lens, int in_mode) {
  static constexpr std::array<ComposeSsKernelFn, kLensIds * kInModes> table =
      compose_ss_cell_table<Interp>(std::make_integer_sequence<int, kLensIds * kInModes>{});
  if (out_lens < 0 || out_lens >= kLensIds || in_mode < 0 || in_mode >= kInModes) return nullptr;
  return table[out_lens * kInModes + in_mode];
}

template <int Interp> hipError_t launch_compose_ss_interp(ComposeSsParams P, int out_lens, int in_mode, hipStream_t stream) {
  P.tiles_x = (P.out_w + kComposeTileW - 1) / kComposeTileW;
  P.tiles_y = (P.out_h + kComposeTileH - 1) / kComposeTileH;
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  const ComposeSsKernelFn fn = compose_ss_cell_kernel<Interp>(out_lens, in_mode);
  if (!fn) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
