// lrp_camstat_packed_kernel.h — the camera overlap statistic of packed frames (include/lrp.h "calibrated cameras, packed pixels",
// DESIGN.md section 21): lrp_camera_overlap_device's table — for every pair of cameras i, j the number of output pixels both see
// with a luminance inside [lo, hi], and the sum of camera i's luminance over them, as 64-bit integers — from frames of 8-bit or
// binary16 samples, in one launch and with no float32 frame.  Included by lrp_camstat_packed.hip alone: the sampler is fixed
// (bilinear), so there is one instantiation per target lens and source format.
//
// It is cam_overlap_kernel (lrp_camstat_kernel.h) with the decoding tap loader PackedTaps (lrp_packed_kernel.h) in place of
// FloatTaps; the body is written out here once more and an edit to it there belongs here too.  The luminance reads the first
// min(C, 3) channels, so a texel is four lanes wide whatever C is, and only min(in_channels, C, 3) samples of a tap are decoded.
//
// Mapping (gfx950): cam_overlap_kernel's, rule by rule — no lane returns before the end, q_i is parked in LDS, the wave's table
// lives across its lanes and is summed by butterflies, one 64-bit vector atomic per non-zero word at the workgroup's end.  What
// is added: the 8-bit decode table in LDS (1 KiB), loaded by the 256 threads in front of the tile loop, with one barrier there.
// LDS in all: 12 KiB for half frames, 13 KiB for 8-bit ones.
#pragma once

#include "lrp_camera_kernel.h"
#include "lrp_camera_packed.h"
#include "lrp_camstat_reduce.h"
#include "lrp_packed_kernel.h"

namespace lrp {

using CameraStatPackedKernelFn = void (*)(const CameraStatPackedParams);

template <int OutLens, int Fmt>
__global__ __launch_bounds__(kComposeThreads) void cam_overlap_packed_kernel(const CameraStatPackedParams P) {
  static_assert(kComposeThreads == 256, "one thread per entry of the 8-bit table");
  __shared__ unsigned long long part[kOverlapWaves][kOverlapWords];
  __shared__ uint32_t parked[kComposeMaxSources][kComposeThreads]; // q_i of this thread's pixel
  __shared__ float lut[256];
  static_assert(sizeof(part) + sizeof(parked) == kOverlapLdsBytes, "the LDS the design states");
  if constexpr (Fmt == kPackedU8) {
    lut[threadIdx.x] = P.decode[threadIdx.x];
    __syncthreads();
  }
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
          Q.channels = 1; // the samplers' element offsets are texel indices (PackedTaps)
          Q.ch_count = P.ch_count;
          Texel<4> s;
          if ((P.in_vec >> i) & 1u) // this camera's taps: one dword / 8-byte load, or one load per sample
            s = sample<1, 4, false>(Q, sx, sy, PackedTaps<Fmt, true>{lut, (uint32_t)P.in_pitch, P.in_copy});
          else
            s = sample<1, 4, false>(Q, sx, sy, PackedTaps<Fmt, false>{lut, (uint32_t)P.in_pitch, P.in_copy});
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

template <int Fmt, int... OutLens>
constexpr std::array<CameraStatPackedKernelFn, kLensIds> camera_stat_packed_kernel_table(std::integer_sequence<int, OutLens...>) {
  return {{cam_overlap_packed_kernel<OutLens, Fmt>...}};
}
// The kernel of output lens out_lens and source format Fmt; nullptr: no such lens.
template <int Fmt> CameraStatPackedKernelFn camera_stat_packed_kernel(int out_lens) {
  static constexpr std::array<CameraStatPackedKernelFn, kLensIds> table =
      camera_stat_packed_kernel_table<Fmt>(std::make_integer_sequence<int, kLensIds>{});
  if (out_lens < 0 || out_lens >= kLensIds) return nullptr;
  return table[out_lens];
}

} // namespace lrp
