// lrp_multiband_label.hip — the label kernel of multi-band blending (include/lrp.h "multi-band blending across a camera rig",
// DESIGN.md section 22): per output pixel the covering camera with the largest FEATHER weight, and the number of covering
// cameras.  One instantiation per target lens; no image is read.
//
// Per output pixel: the geometry of compose_cam_kernel (lrp_camera_kernel.h) at num_samples == 1 — IdealTarget<OutLens>, the
// rotation, CameraSources::map (camera_project and the box test) are that kernel's, restated nowhere — and FEATHER's w_i in the
// arithmetic of compose_ss_pixel (lrp_compose_pixel.h).  The winner: cameras in ascending i, replaced on w_i > best, so a tie
// goes to the lowest index.
//
// Mapping (gfx950): compose_cam_kernel's 32 x 8 tile, one pixel per lane, tiles in xcd_tile() order, descriptors in SGPRs, the
// camera loop rolled.  Two byte stores per lane; no LDS.
#include <hip/hip_runtime.h>

#include "lrp_camera_kernel.h"
#include "lrp_multiband.h"

namespace lrp {

using MultibandLabelKernelFn = void (*)(const MultibandLabelParams);

template <int OutLens>
__global__ __launch_bounds__(kComposeThreads) void multiband_label_kernel(const MultibandLabelParams P) {
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;
  const IdealTarget<OutLens> T(P, x, y);
  const float ns1 = 2.0f; // num_samples + 1
  float rx, ry, rz;
  T.ray(P, T.column(0, ns1), 0, ns1, rx, ry, rz);

  uint32_t k = 0, winner = (uint32_t)kMultibandNoCamera;
  float best = 0.0f;
#pragma unroll 1
  for (int i = 0; i < P.n_src; ++i) {
    const CameraSource &S = P.src[i]; // wave-uniform
    float vx = rx, vy = ry, vz = rz;
    if (S.has_rot) {
      vx = S.rot[0] * rx + S.rot[1] * ry + S.rot[2] * rz;
      vy = S.rot[3] * rx + S.rot[4] * ry + S.rot[5] * rz;
      vz = S.rot[6] * rx + S.rot[7] * ry + S.rot[8] * rz;
    }
    const float in_w = (float)S.in_w, in_h = (float)S.in_h;
    float sx, sy;
    if (!CameraSources::map(S, vx, vy, vz, in_w, in_h, sx, sy)) continue;
    const float dy = compose_min(sy + 0.5f, (in_h - 0.5f) - sy);
    const float d = compose_min(compose_min(sx + 0.5f, (in_w - 0.5f) - sx), dy);
    const float w = (d < 0x1p-10f) ? 0x1p-10f : d;
    if (k == 0u || w > best) best = w, winner = (uint32_t)i;
    k += 1u;
  }
  const uint32_t px_index = (uint32_t)y * (uint32_t)P.out_w + (uint32_t)x;
  P.label[px_index] = (uint8_t)winner;
  P.count[px_index] = (uint8_t)k;
}

template <int... OutLens>
constexpr std::array<MultibandLabelKernelFn, kLensIds> multiband_label_table(std::integer_sequence<int, OutLens...>) {
  return {{multiband_label_kernel<OutLens>...}};
}

hipError_t launch_multiband_label(const MultibandLabelParams &P, int out_lens, hipStream_t stream) {
  static constexpr std::array<MultibandLabelKernelFn, kLensIds> table = multiband_label_table(std::make_integer_sequence<int, kLensIds>{});
  if (P.n_src < 1 || P.n_src > kComposeMaxSources || out_lens < 0 || out_lens >= kLensIds) return hipErrorInvalidValue;
  MultibandLabelParams Q = P;
  return launch_compose_tiles(table[out_lens], Q, Q, stream);
}

} // namespace lrp
