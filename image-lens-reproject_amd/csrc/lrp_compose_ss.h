// lrp_compose_ss.h — kernel argument block of the supersampled compose kernel (lrp_compose_ss_kernel.h; include/lrp.h
// "compose, supersampled"), shared by lrp_capi.cpp and the lrp_compose_ss*.hip units.  The fields of
// ComposeParams (lrp_compose.h) plus num_samples and the coverage plane; a block of its own, so that ComposeParams — and with
// it the kernarg layout, the bytes and the time of lrp_compose_device — does not move.  Plain POD passed by value in kernarg:
// wave-uniform, read with scalar loads.
#pragma once

#include <stdint.h>

#include "lrp_compose.h"

namespace lrp {

constexpr int kComposeSsMaxSamples = 15; // num_samples of include/lrp.h: n * n <= 225 fits the coverage plane's byte

struct ComposeSsParams {
  float *dst;
  uint8_t *count;      // the plane of the number of sources that cover at least one sub-sample, or null
  uint8_t *coverage;   // the plane of m, the number of covered sub-samples (0 .. n * n), or null
  int32_t out_w, out_h;
  int32_t channels;    // floats per texel (the stride), every source's and the output's
  int32_t ch_count;    // channels composed by this launch (<= kMaxDynChannels; dst and the sources' data point at the first)
  int32_t n_src;       // 1 .. kComposeMaxSources
  int32_t mode;        // kComposeFirst / kComposeMean / kComposeFeather
  int32_t num_samples; // n: 1 .. kComposeSsMaxSamples sub-samples per axis
  int32_t has_post;    // fused post_process on the composed value
  float exposure, reinhard;
  int32_t tiles_x, tiles_y; // output tiling (lrp_kernel_impl.h: 32 x 8 pixels, xcd_tile numbering)
  LensP out_lens;
  ComposeSource src[kComposeMaxSources];
};

} // namespace lrp
