// lrp_camstat.h — kernel argument block of the camera overlap statistic (lrp_camstat_kernel.h; include/lrp.h "exposure matching
// across a camera rig"), shared by lrp_capi.cpp and lrp_camstat.hip.  The camera descriptors are
// lrp_camera.h's CameraSource; the rest is what a reduction needs instead of an output image.  Plain POD passed by value in
// kernarg: wave-uniform, read with scalar loads.
#pragma once

#include <stdint.h>

#include "lrp_camera.h"

namespace lrp {

constexpr int kOverlapWords = 2 * kComposeMaxSources * kComposeMaxSources; // LRP_OVERLAP_WORDS
// Most workgroups of one launch: every workgroup ends with at most 2 * n_src^2 atomic adds into the same 1 KB, so their number
// is bounded and a workgroup walks several tiles.  A multiple of kXcds, so that workgroup % kXcds — the
// XCD of xcd_tile() — is the same for every tile a workgroup walks.
constexpr int kOverlapMaxBlocks = 2048;

struct CameraStatParams {
  unsigned long long *stats; // kOverlapWords words, zeroed ahead of the launch
  int32_t out_w, out_h;
  int32_t channels;          // floats per texel of every camera (the stride)
  int32_t ch_count;          // min(channels, 3): the channels the luminance reads
  int32_t n_src;             // 1 .. kComposeMaxSources
  float lo, hi;              // 0 <= lo <= hi <= 32768
  int32_t tiles_x, tiles_y;  // output tiling (32 x 8 pixels, xcd_tile numbering)
  int32_t n_groups;          // workgroup numbers of the tiling: kXcds * xcd_rows(tiles_y) * tiles_x
  LensP out_lens;
  CameraSource src[kComposeMaxSources];
};

} // namespace lrp
