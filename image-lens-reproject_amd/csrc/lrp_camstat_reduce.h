// lrp_camstat_reduce.h — what the two overlap kernels share of their reduction (lrp_camstat_kernel.h, lrp_camstat_packed_kernel.h;
// DESIGN.md sections 19 and 21): the LDS both state and the wave-wide sum.  A header of its own so that a unit of one kernel
// family does not instantiate the other's kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "lrp_camstat.h"
#include "lrp_compose_kernel.h"

namespace lrp {

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

} // namespace lrp
