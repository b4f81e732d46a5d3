// lrp_lanczos.hip — the Lanczos-3 sampler (include/lrp.h "Lanczos-3"): the launcher lrp_capi.cpp calls
// and the computing instantiations of lrp_lanczos_kernel.h, one per cell.  The kernels that read a geometry-cache entry are
// lrp_lanczos_geo.hip.
#include <hip/hip_runtime.h>

#include "lrp_lanczos_kernel.h"

namespace lrp {

hipError_t launch_lanczos_geo(const KParams &P, dim3 grid, int in_mode, hipStream_t stream);

// P: as make_params() filled it, the caller's band, channel group and geometry-cache use applied.  P.channels == 4 takes the
// RGBA instantiations, anything else the run-time channel path (P.ch_count <= 8 channels at stride P.channels).
hipError_t launch_lanczos(KParams P, int out_lens, int in_mode, hipStream_t stream) {
  if (P.num_samples < 1 || P.ch_count < 1 || P.ch_count > kMaxDynChannels || (P.geo_mode != 0 && (P.geo_xy == nullptr || P.num_samples != 1)))
    return hipErrorInvalidValue;
  dim3 grid;
  if (!lanczos_grid(P, grid)) return hipSuccess;
  if (P.geo_mode == 2) return launch_lanczos_geo(P, grid, in_mode, stream);
  const KernelFn fn = P.channels == 4 ? cell_kernel<LanczosCell<4>>(out_lens, in_mode) : cell_kernel<LanczosCell<0>>(out_lens, in_mode);
  if (!fn) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fn, grid, dim3(kLzThreads), 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
