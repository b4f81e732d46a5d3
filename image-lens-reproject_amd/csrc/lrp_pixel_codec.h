// lrp_pixel_codec.h — the 8-bit encode of one sample (include/lrp.h LRP_PIXEL_U8_GAMMA) for the kernel that stores packed pixels
// itself (lrp_packed_kernel.h): the clamp and the threshold search of encode_kernel (lrp_pixel_kernels.hip), statement for
// statement.  (encode_kernel keeps its own copy: routed through this header its machine code differs from the parent's, and
// tests/test_gpu_packed.py compares the two byte for byte.)  The table is the host's (host_tables): no device pow is involved.
#pragma once

#include <hip/hip_runtime.h>

namespace lrp {

// std::max(0.0f, std::min(1.0f, s)) with libstdc++'s comparison direction: NaN -> 1, -0 -> +0
__device__ __forceinline__ float unit_clamp_png(float v) {
  const float m = (v < 1.0f) ? v : 1.0f;
  return (0.0f < m) ? m : 0.0f;
}

// The 8-bit code of v.  thr: the 256 thresholds (threshold[k] = smallest s in [0, 1] whose code is >= k, threshold[0] = 0), in LDS.
__device__ __forceinline__ int u8_gamma_code(const float *thr, float v) {
  const float s = unit_clamp_png(v);
  // code = number of thresholds 1..255 that s has reached (thr is non-decreasing): 8 halving steps
  int lo = 0, hi = 256; // invariant: thr[lo] <= s (thr[0] = 0), s < thr[hi] (thr[256] = +inf)
#pragma unroll
  for (int step = 0; step < 8; ++step) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= s)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

} // namespace lrp
