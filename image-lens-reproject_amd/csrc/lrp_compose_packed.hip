// lrp_compose_packed.hip — several packed sources composed into one packed output by one launch (include/lrp.h "compose, packed
// pixels"): the launcher lrp_capi.cpp calls, and the nearest-neighbour instantiations of
// compose_packed_kernel (lrp_compose_packed_kernel.h).  The bilinear ones and, one source format each, the bicubic ones
// are units of lrp_compose_packed_unit.hip (units.list).
#include <hip/hip_runtime.h>

#include "lrp_compose_packed_kernel.h"

namespace lrp {

hipError_t pixel_tables_device(int device, hipStream_t stream, const float **decode, const float **threshold); // lrp_pixel_kernels.hip

// P: what lrp_capi.cpp states (lrp_compose_packed.h); the rest is derived here.  in_format: kPackedF16 / kPackedU8.
// interpolation: 0 nearest, 1 bilinear, 2 bicubic (include/lrp.h lrp_interpolation).
hipError_t launch_compose_packed(ComposePackedParams P, int in_format, int out_lens, int in_mode, int interpolation, int device, hipStream_t stream) {
  if ((in_format != kPackedF16 && in_format != kPackedU8) || (P.out_format != kPackedF32 && P.out_format != kPackedF16 && P.out_format != kPackedU8) ||
      P.n_src < 1 || P.n_src > kComposeMaxSources || P.channels < 1 || P.channels > kPackedMaxChannels || P.in_channels < 1 || P.out_channels < 1)
    return hipErrorInvalidValue;
  const hipError_t e = pixel_tables_device(device, stream, &P.decode, &P.threshold);
  if (e != hipSuccess) return e;
  const int in_sample = in_format == kPackedU8 ? 1 : 2, out_sample = P.out_format == kPackedU8 ? 1 : (P.out_format == kPackedF16 ? 2 : 4);
  P.in_pitch = P.in_channels * in_sample;
  P.out_pitch = P.out_channels * out_sample;
  P.in_copy = P.in_channels < P.channels ? P.in_channels : P.channels;
  P.out_copy = P.channels < P.out_channels ? P.channels : P.out_channels;
  for (int i = 0; i < P.n_src; ++i) // per source: base pointers differ in alignment within one call
    P.src[i].in_vec = P.in_channels == 4 && reinterpret_cast<uintptr_t>(P.src[i].data) % (uintptr_t)(4 * in_sample) == 0;
  P.out_vec = P.out_channels == 4 && reinterpret_cast<uintptr_t>(P.dst) % (uintptr_t)(4 * out_sample) == 0;
  P.tiles_x = (P.out_w + kComposeTileW - 1) / kComposeTileW;
  P.tiles_y = (P.out_h + kComposeTileH - 1) / kComposeTileH;
  if (interpolation == 0) return launch_compose_packed_interp<0>(P, in_format, out_lens, in_mode, stream);
  if (interpolation == 1)
    return in_format == kPackedU8 ? launch_compose_packed_unit<1, kPackedU8>(P, out_lens, in_mode, stream) : launch_compose_packed_unit<1, kPackedF16>(P, out_lens, in_mode, stream);
  if (interpolation == 2)
    return in_format == kPackedU8 ? launch_compose_packed_unit<2, kPackedU8>(P, out_lens, in_mode, stream) : launch_compose_packed_unit<2, kPackedF16>(P, out_lens, in_mode, stream);
  return hipErrorInvalidValue;
}

} // namespace lrp
