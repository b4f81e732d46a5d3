// lrp_camstat.hip — the camera overlap statistic by one launch (include/lrp.h "exposure matching across a camera rig", DESIGN.md
// section 19): the launcher lrp_capi.cpp calls, and the five instantiations of cam_overlap_kernel (lrp_camstat_kernel.h), one per
// target lens.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "lrp_camstat_kernel.h"

namespace lrp {

// P: everything but the tiling.  The table is zeroed on `stream` ahead of the kernel, which adds into it; the host does not
// synchronise.
hipError_t launch_camera_overlap(const CameraStatParams &P0, int out_lens, hipStream_t stream) {
  CameraStatParams P = P0;
  if (P.n_src < 1 || P.n_src > kComposeMaxSources || P.ch_count < 1 || P.ch_count > 3 || P.stats == nullptr) return hipErrorInvalidValue;
  const CameraStatKernelFn fn = camera_stat_kernel(out_lens);
  if (!fn) return hipErrorInvalidValue;
  const hipError_t e = hipMemsetAsync(P.stats, 0, sizeof(unsigned long long) * kOverlapWords, stream);
  if (e != hipSuccess) return e;
  P.tiles_x = (P.out_w + kComposeTileW - 1) / kComposeTileW;
  P.tiles_y = (P.out_h + kComposeTileH - 1) / kComposeTileH;
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  P.n_groups = kXcds * xcd_rows(P.tiles_y) * P.tiles_x;
  const dim3 grid((unsigned)std::min(P.n_groups, kOverlapMaxBlocks)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
