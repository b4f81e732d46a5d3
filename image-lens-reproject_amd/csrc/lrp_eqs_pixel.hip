// lrp_eqs_pixel.hip — the one-pixel-per-lane kernel for the equisolid cells (lrp_eqs.h): three samplers, RGBA and the
// run-time channel path (any channel count, images of 4 GiB and more).
#include "lrp_eqs.h"
#include "lrp_kernel_impl.h"

namespace lrp {
namespace {
template <int Interp, bool OutEqs> struct EqsPixelPick {
  static KernelFn get(const KParams &P, int out_idx, int in_mode) {
#define LRP_K4(O, I) reproject_kernel<O, I, Interp, 4>
#define LRP_K0(O, I) reproject_kernel<O, I, Interp, 0>
    static const KernelFn t4[kEqsCells] = LRP_EQS_CELL_TABLE(LRP_K4);
    static const KernelFn t0[kEqsCells] = LRP_EQS_CELL_TABLE(LRP_K0);
#undef LRP_K4
#undef LRP_K0
    const int cell = eqs_cell_of_index(OutEqs, out_idx, in_mode);
    if (cell < 0) return nullptr;
    return P.channels == 4 ? t4[cell] : t0[cell];
  }
};
} // namespace

namespace {
template <bool OutEqs> hipError_t launch_eqs_pixel_impl(const KParams &P, int interpolation, int out_idx, int in_mode, hipStream_t stream) {
  if (interpolation == 0) return launch_interp<0, EqsPixelPick<0, OutEqs>>(P, out_idx, in_mode, stream);
  if (interpolation == 1) return launch_interp<1, EqsPixelPick<1, OutEqs>>(P, out_idx, in_mode, stream);
  return launch_interp<2, EqsPixelPick<2, OutEqs>>(P, out_idx, in_mode, stream);
}
hipError_t launch_eqs_pixel(const KParams &P, int interpolation, int out_lens, int in_mode, hipStream_t stream) {
  if (out_lens == kEquisolid) return launch_eqs_pixel_impl<true>(P, interpolation, eqs_out_index(out_lens), in_mode, stream);
  return launch_eqs_pixel_impl<false>(P, interpolation, eqs_out_index(out_lens), in_mode, stream);
}
const bool g_registered = (g_eqs_launchers.pixel = launch_eqs_pixel, true);
} // namespace
} // namespace lrp
