// lrp_compose.h — kernel argument block of the compose kernel (lrp_compose_kernel.h; include/lrp.h "compose", DESIGN.md
// section 12), shared by lrp_capi.cpp and the lrp_compose*.hip units.  Plain POD passed by value in kernarg like KParams
// (lrp_params.h): wave-uniform, read with scalar loads — the source loop indexes `src` with a wave-uniform counter.
#pragma once

#include <stdint.h>

#include "lrp_params.h"

namespace lrp {

constexpr int kComposeMaxSources = 8; // LRP_COMPOSE_MAX_SOURCES
constexpr int kComposeMaxChannels = 8; // channels per launch: the run-time channel path of lrp_device.h (kMaxDynChannels)
enum : int { kComposeFirst = 0, kComposeMean = 1, kComposeFeather = 2 }; // lrp_compose_mode

// One source image: what ray_to_source / sample<> of lrp_device.h read of KParams for it.  (The lens-only constants of
// KParams — in_focal, in_lon_span ... — belong to the tile kernel; the lens functions used here derive them per pixel,
// like the one-pixel-per-lane kernel.)
struct ComposeSource {
  const float *data;
  int32_t in_w, in_h;
  LensP lens;
  int32_t has_rot;
  float rot[9]; // row-major; valid when has_rot
};

struct ComposeParams {
  float *dst;
  uint8_t *count;      // the plane of k (out_w * out_h bytes, any alignment), or null
  int32_t out_w, out_h;
  int32_t channels;    // floats per texel (the stride), every source's and the output's
  int32_t ch_count;    // channels composed by this launch (<= kMaxDynChannels; dst and the sources' data point at the first)
  int32_t n_src;       // 1 .. kComposeMaxSources
  int32_t mode;        // kComposeFirst / kComposeMean / kComposeFeather
  int32_t has_post;    // fused post_process on the composed value
  float exposure, reinhard;
  int32_t tiles_x, tiles_y; // output tiling (lrp_kernel_impl.h: 32 x 8 pixels, xcd_tile numbering)
  LensP out_lens;
  ComposeSource src[kComposeMaxSources];
};

} // namespace lrp
