// lrp_camstat_kernel.h — the camera overlap statistic (include/lrp.h "exposure matching across a camera rig", DESIGN.md section
// 19): for every pair of cameras i, j the number of output pixels both see with a luminance inside [lo, hi], and the sum of
// camera i's luminance over them, as 64-bit integers — one launch, no image.  Included by lrp_camstat.hip alone: the sampler
// is fixed (bilinear), so there is one instantiation per target lens.
//
// Per output pixel: the pixel centre of compose_cam_kernel (lrp_camera_kernel.h) at num_samples == 1 — target_ray, the rotation,
// camera_project, the coverage test and sample<1> are that kernel's, restated nowhere — then Y_i, valid_i and q_i of the header.
//
// Mapping (gfx950): compose_cam_kernel's 32 x 8 tile, one pixel per lane, tiles in xcd_tile() order, descriptors in SGPRs, a
// ballot per camera so that a camera no lane sees forms no address.  What a reduction changes:
//   - no lane returns before the end.  Lanes outside the image and workgroup numbers xcd_tile() rejects take part with every
//     valid bit clear: the wave-wide sums and the barrier below see all 256 lanes.
//   - the per-lane state is eight q_i and an 8-bit mask.  The mask is a register; q_i is parked in LDS, each lane in a slot of
//     its own (8 cameras x 256 lanes x 4 bytes = 8 KB; no barrier: a lane reads back what it wrote).  The camera loop stays
//     rolled like compose_cam_kernel's: unrolled eight times, the descriptors of all cameras are live at once and the SGPRs spill.
//   - a workgroup walks tiles g = blockIdx.x, blockIdx.x + gridDim.x, .. and adds to memory once, at its end: at most
//     kOverlapMaxBlocks x 2 n^2 atomic adds per launch instead of 2 n^2 per tile, all of which land in the same 1 KB.
//   - the wave's table lives across its lanes: lane i * 8 + j owns entry (i, j) and keeps N_ij, S_ij in two 64-bit registers.
//     N_ij of a tile is the population count of a ballot (scalar); S_ij a butterfly sum of q_i over the lanes of that ballot,
//     in two 16-bit halves so that 64 values of up to 2^31 cannot overflow 32 bits.  A pair no lane of the wave has is skipped.
//   - at the end the four waves' tables meet in LDS (4 waves x 128 words x 8 bytes = 4 KB), one barrier, and threads 0 .. 127 add
//     the non-zero words with one 64-bit vector atomic each (agent scope).  LDS in all: 12 KB (kOverlapLdsBytes).
// Integer sums: the result is the same whatever the order.  Nothing is accumulated in float.
#pragma once

#include "lrp_camera_kernel.h"
#include "lrp_camstat.h"

namespace lrp {

using CameraStatKernelFn = void (*)(const CameraStatParams);

constexpr int kOverlapWaves = kComposeThreads / 64;
constexpr int kOverlapLdsBytes = kComposeMaxSources * kComposeThreads * 4 + kOverlapWaves * kOverlapWords * 8; // 8 KB + 4 KB
static_assert(kOverlapWords == 2 * 64 && kComposeThreads >= kOverlapWords && kOverlapMaxBlocks % kXcds == 0,
              "one lane per table entry, one thread per table word, a workgroup stays on its XCD");

// The sum of v over the wave's 64 lanes, in every lane.  Every lane of the wave executes it.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}

template <int OutLens>
__global__ __launch_bounds__(kComposeThreads) void cam_overlap_kernel(const CameraStatParams P) {
  __shared__ unsigned long long part[kOverlapWaves][kOverlapWords];
  __shared__ uint32_t parked[kComposeMaxSources][kComposeThreads]; // q_i of this thread's pixel
  static_assert(sizeof(part) + sizeof(parked) == kOverlapLdsBytes, "the LDS the design states");
  const int lane = (int)(threadIdx.x % 64u), wave = (int)(threadIdx.x / 64u);
  unsigned long long acc_n = 0ull, acc_s = 0ull; // entry (lane / 8, lane % 8) of this wave's table

#pragma unroll 1
  for (uint32_t g = blockIdx.x; g < (uint32_t)P.n_groups; g += gridDim.x) { // workgroup-uniform
    int tx, ty;
    if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty, g)) continue; // the whole workgroup
    const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
    const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
    const bool inside = x < P.out_w && y < P.out_h; // a lane outside stays, with no valid bit

    // pixel centre in image-centred coordinates, and the one sub-sample of n == 1: cx + (0 + 1) / (1 + 1) - 0.5
    const float cx = ((float)x + 0.5f) - (float)P.out_w * 0.5f;
    const float cy = ((float)y + 0.5f) - (float)P.out_h * 0.5f;
    const float scx = (cx + 0.5f) - 0.5f;
    const float scy = (cy + 0.5f) - 0.5f;
    float rx, ry, rz;
    target_ray<OutLens>(P.out_lens, (float)P.out_w, (float)P.out_h, scx, scy, rx, ry, rz);

    uint32_t valid = 0; // bit i: valid_i
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
      const bool covered = inside && imaged && sx >= -0.5f && sx <= in_w - 0.5f && sy >= -0.5f && sy <= in_h - 0.5f;
      uint32_t q = 0u;
      if (__builtin_amdgcn_ballot_w64(covered) != 0ull) { // a camera no lane sees is not sampled
        if (covered) {
          KParams Q; // the sampler's view of camera i (sample<> reads these five fields)
          Q.src = S.data;
          Q.in_w = S.in_w;
          Q.in_h = S.in_h;
          Q.channels = P.channels;
          Q.ch_count = P.ch_count;
          const Texel<0> s = sample<1, 0, false>(Q, sx, sy);
          float Y = s.v[0];
          if (P.ch_count >= 3) Y = (0.25f * s.v[0] + 0.5f * s.v[1]) + 0.25f * s.v[2];
          if (Y >= P.lo && Y <= P.hi) { // false for NaN
            q = (uint32_t)(Y * 65536.0f); // exact, at most 2^31
            valid |= 1u << i;
          }
        }
      }
      parked[i][threadIdx.x] = q;
    }

    // this tile into the wave's table: every pair some lane has
#pragma unroll 1
    for (int i = 0; i < P.n_src; ++i) {
      if (__builtin_amdgcn_ballot_w64(((valid >> i) & 1u) != 0u) == 0ull) continue; // wave-uniform: no lane has valid_i
      const uint32_t qi = parked[i][threadIdx.x];
#pragma unroll 1
      for (int j = 0; j < P.n_src; ++j) {
        const bool both = ((valid >> i) & (valid >> j) & 1u) != 0u;
        const unsigned long long b = __builtin_amdgcn_ballot_w64(both);
        if (b == 0ull) continue; // wave-uniform
        const uint32_t v = both ? qi : 0u;
        const uint32_t lo16 = wave_sum_u32(v & 0xFFFFu); // < 2^22
        const uint32_t hi16 = wave_sum_u32(v >> 16);     // < 2^22
        if (lane == i * kComposeMaxSources + j) {
          acc_n += (unsigned long long)__builtin_popcountll(b);
          acc_s += (unsigned long long)lo16 + ((unsigned long long)hi16 << 16);
        }
      }
    }
  }

  // the four waves' tables -> one, and at most one atomic per word
  part[wave][2 * lane] = acc_n;
  part[wave][2 * lane + 1] = acc_s;
  __syncthreads();
  if (threadIdx.x < (unsigned)kOverlapWords) {
    unsigned long long sum = 0ull;
#pragma unroll
    for (int w = 0; w < kOverlapWaves; ++w) sum += part[w][threadIdx.x];
    if (sum != 0ull) atomicAdd(P.stats + threadIdx.x, sum);
  }
}

template <int... OutLens>
constexpr std::array<CameraStatKernelFn, kLensIds> camera_stat_kernel_table(std::integer_sequence<int, OutLens...>) {
  return {{cam_overlap_kernel<OutLens>...}};
}
// The kernel of output lens out_lens; nullptr: no such lens.
inline CameraStatKernelFn camera_stat_kernel(int out_lens) {
  static constexpr std::array<CameraStatKernelFn, kLensIds> table = camera_stat_kernel_table(std::make_integer_sequence<int, kLensIds>{});
  if (out_lens < 0 || out_lens >= kLensIds) return nullptr;
  return table[out_lens];
}

} // namespace lrp
