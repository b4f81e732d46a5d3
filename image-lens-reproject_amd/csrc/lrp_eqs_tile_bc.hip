// lrp_eqs_tile_bc.hip — bicubic instantiations of the tile kernel for the equisolid cells (lrp_eqs_tile.h).
#include "lrp_eqs_tile.h"

namespace lrp {
namespace {
hipError_t launch_eqs_tile_bicubic(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_eqs_tile<2>(P, out_lens, in_mode, stream);
}
const bool g_registered = (g_eqs_launchers.tile[2] = launch_eqs_tile_bicubic, true);
} // namespace
} // namespace lrp
