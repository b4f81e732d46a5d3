// lrp_multiband.hip — the pyramid kernels of multi-band blending (lrp_multiband_kernel.h; include/lrp.h "multi-band blending
// across a camera rig"), instantiated for 1 .. 4 colour channels, and the launchers lrp_capi.cpp calls.
// The label kernel is lrp_multiband_label.hip.
#include <hip/hip_runtime.h>

#include "lrp_multiband_kernel.h"

namespace lrp {

namespace {

// One workgroup per 32 x 8 tile of the w x h level the kernel writes.  An empty level is no error.
template <typename Args> hipError_t launch_level(void (*fn)(const Args), const Args &A, int w, int h, hipStream_t stream) {
  if (w <= 0 || h <= 0) return hipSuccess;
  const dim3 grid((unsigned)((w + kMbTileW - 1) / kMbTileW), (unsigned)((h + kMbTileH - 1) / kMbTileH)), block(kMbThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, A);
  return hipGetLastError();
}

} // namespace

hipError_t launch_multiband_reduce(const MultibandReduceParams &P, int channels, hipStream_t stream) {
  static constexpr void (*table[kMultibandMaxChannels])(const MultibandReduceParams) = {
      multiband_reduce_kernel<1>, multiband_reduce_kernel<2>, multiband_reduce_kernel<3>, multiband_reduce_kernel<4>};
  if (channels < 1 || channels > kMultibandMaxChannels) return hipErrorInvalidValue;
  return launch_level(table[channels - 1], P, P.cw, P.ch, stream);
}

hipError_t launch_multiband_lap(const MultibandLapParams &P, int channels, hipStream_t stream) {
  static constexpr void (*table[kMultibandMaxChannels])(const MultibandLapParams) = {
      multiband_lap_kernel<1>, multiband_lap_kernel<2>, multiband_lap_kernel<3>, multiband_lap_kernel<4>};
  if (channels < 1 || channels > kMultibandMaxChannels) return hipErrorInvalidValue;
  return launch_level(table[channels - 1], P, P.w, P.h, stream);
}

hipError_t launch_multiband_collapse(const MultibandCollapseParams &P, int channels, hipStream_t stream) {
  static constexpr void (*table[kMultibandMaxChannels])(const MultibandCollapseParams) = {
      multiband_collapse_kernel<1>, multiband_collapse_kernel<2>, multiband_collapse_kernel<3>, multiband_collapse_kernel<4>};
  if (channels < 1 || channels > kMultibandMaxChannels) return hipErrorInvalidValue;
  return launch_level(table[channels - 1], P, P.w, P.h, stream);
}

} // namespace lrp
