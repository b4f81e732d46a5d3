// lrp_camstat_packed.hip — the camera overlap statistic of packed frames by one launch (include/lrp.h "calibrated cameras, packed
// pixels"): the launcher lrp_capi.cpp calls, and the ten instantiations of cam_overlap_packed_kernel
// (lrp_camstat_packed_kernel.h), one per target lens and source format.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lrp_camstat_packed_kernel.h"

namespace lrp {

hipError_t pixel_tables_device(int device, hipStream_t stream, const float **decode, const float **threshold); // lrp_pixel_kernels.hip

// P: what lrp_capi.cpp states (lrp_camera_packed.h); the rest is derived here.  in_format: kPackedF16 / kPackedU8.  The table
// is zeroed on `stream` ahead of the kernel, which adds into it; the host does not synchronise.
hipError_t launch_camera_overlap_packed(CameraStatPackedParams P, int in_format, int out_lens, int device, hipStream_t stream) {
  if ((in_format != kPackedF16 && in_format != kPackedU8) || P.n_src < 1 || P.n_src > kComposeMaxSources || P.channels < 1 || P.in_channels < 1 ||
      P.stats == nullptr)
    return hipErrorInvalidValue;
  const CameraStatPackedKernelFn fn = in_format == kPackedU8 ? camera_stat_packed_kernel<kPackedU8>(out_lens) : camera_stat_packed_kernel<kPackedF16>(out_lens);
  if (!fn) return hipErrorInvalidValue;
  const float *threshold = nullptr;
  hipError_t e = pixel_tables_device(device, stream, &P.decode, &threshold);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(P.stats, 0, sizeof(unsigned long long) * kOverlapWords, stream);
  if (e != hipSuccess) return e;
  const int in_sample = in_format == kPackedU8 ? 1 : 2;
  P.ch_count = std::min(P.channels, 3);
  P.in_pitch = P.in_channels * in_sample;
  P.in_copy = std::min(P.in_channels, P.ch_count);
  P.in_vec = 0u;
  for (int i = 0; i < P.n_src; ++i) // per camera: base pointers differ in alignment within one call
    if (P.in_channels == 4 && reinterpret_cast<uintptr_t>(P.src[i].data) % (uintptr_t)(4 * in_sample) == 0) P.in_vec |= 1u << i;
  P.tiles_x = (P.out_w + kComposeTileW - 1) / kComposeTileW;
  P.tiles_y = (P.out_h + kComposeTileH - 1) / kComposeTileH;
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  P.n_groups = kXcds * xcd_rows(P.tiles_y) * P.tiles_x;
  const dim3 grid((unsigned)std::min(P.n_groups, kOverlapMaxBlocks)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
