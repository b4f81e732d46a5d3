// lrp_tile_wing5.hip — bicubic window-kernel instantiations (lrp_kernel_v2.h): RGBAZ, coordinates from the geometry cache (GeoRead).
#include "lrp_kernel_v2.h"

namespace lrp {
hipError_t launch_win_bicubic_geo_c5(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_win_bicubic_impl<0, 5, true>(P, out_lens, in_mode, stream);
}
} // namespace lrp
