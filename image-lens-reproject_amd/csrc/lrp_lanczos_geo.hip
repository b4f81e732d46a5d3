// lrp_lanczos_geo.hip — the Lanczos-3 kernels that read a geometry-cache entry (lrp_lanczos_kernel.h lanczos_geo_kernel): no
// lens math, one per <wrapping source, channel path>.  Launcher: lrp_lanczos.hip.
#include <hip/hip_runtime.h>

#include "lrp_lanczos_kernel.h"

namespace lrp {

// Every output lens and every source mode: only whether the source wraps matters (the extension lenses' sources are clamped,
// like geo_read_in_mode's choice for the other samplers).
hipError_t launch_lanczos_geo(const KParams &P, dim3 grid, int in_mode, hipStream_t stream) {
  const bool loop = in_mode == kInEquirectLoop;
  KernelFn fn;
  if (P.channels == 4)
    fn = loop ? lanczos_geo_kernel<true, 4> : lanczos_geo_kernel<false, 4>;
  else
    fn = loop ? lanczos_geo_kernel<true, 0> : lanczos_geo_kernel<false, 0>;
  hipLaunchKernelGGL(fn, grid, dim3(kLzThreads), 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
