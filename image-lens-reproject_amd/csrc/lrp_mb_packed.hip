// lrp_mb_packed.hip — the level-0 collapse of multi-band blending into a packed output (lrp_mb_packed_kernel.h; include/lrp.h
// "multi-band blending, packed pixels"), instantiated for 1 .. 4 colour channels, and the launcher
// lrp_capi.cpp calls.
#include <hip/hip_runtime.h>

#include "lrp_mb_packed_kernel.h"

namespace lrp {

hipError_t pixel_tables_device(int device, hipStream_t stream, const float **decode, const float **threshold); // lrp_pixel_kernels.hip

// P: what lrp_capi.cpp states (lrp_mb_packed.h); the rest is derived here.  One workgroup per 32 x 8 tile of the output.
hipError_t launch_mb_collapse_packed(MbCollapsePackedParams P, int channels, int device, hipStream_t stream) {
  static constexpr void (*table[kMultibandMaxChannels])(const MbCollapsePackedParams) = {
      mb_collapse_packed_kernel<1>, mb_collapse_packed_kernel<2>, mb_collapse_packed_kernel<3>, mb_collapse_packed_kernel<4>};
  if (channels < 1 || channels > kMultibandMaxChannels || P.out_channels < 1 ||
      (P.out_format != kPackedF32 && P.out_format != kPackedF16 && P.out_format != kPackedU8))
    return hipErrorInvalidValue;
  const float *decode = nullptr;
  const hipError_t e = pixel_tables_device(device, stream, &decode, &P.threshold);
  if (e != hipSuccess) return e;
  const int out_sample = P.out_format == kPackedU8 ? 1 : (P.out_format == kPackedF16 ? 2 : 4);
  P.out_pitch = P.out_channels * out_sample;
  P.out_copy = channels < P.out_channels ? channels : P.out_channels;
  P.out_vec = P.out_channels == 4 && reinterpret_cast<uintptr_t>(P.dst) % (uintptr_t)(4 * out_sample) == 0;
  if (P.w <= 0 || P.h <= 0) return hipSuccess;
  const dim3 grid((unsigned)((P.w + kMbTileW - 1) / kMbTileW), (unsigned)((P.h + kMbTileH - 1) / kMbTileH)), block(kMbThreads);
  hipLaunchKernelGGL(table[channels - 1], grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
