// lrp_eqs_tile_nn.hip — nearest instantiations of the tile kernel for the equisolid cells (lrp_eqs_tile.h).
#include "lrp_eqs_tile.h"

namespace lrp {
namespace {
hipError_t launch_eqs_tile_nearest(const KParams &P, int out_lens, int in_mode, hipStream_t stream) {
  return launch_eqs_tile<0>(P, out_lens, in_mode, stream);
}
const bool g_registered = (g_eqs_launchers.tile[0] = launch_eqs_tile_nearest, true);
} // namespace
} // namespace lrp
