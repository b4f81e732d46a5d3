// lrp_compose_packed.h — kernel argument block of the packed compose kernel (lrp_compose_packed_kernel.h; include/lrp.h "compose,
// packed pixels"), shared by lrp_capi.cpp and the lrp_compose_packed*.hip units.  Plain POD passed by value
// in kernarg like ComposeParams (lrp_compose.h) and PackedParams (lrp_packed.h): wave-uniform, read with scalar loads — the
// source loop indexes `src` with a wave-uniform counter.
#pragma once

#include <stdint.h>

#include "lrp_compose.h"
#include "lrp_packed.h"

namespace lrp {

// One source image: ComposeSource (lrp_compose.h) with packed samples behind `data`, and whether ITS taps take the one-load
// path — base pointers differ in alignment from source to source within one call.
struct ComposePackedSource {
  const void *data; // in_w x in_h texels of in_channels packed samples (binary16 or 8-bit; the format is a template argument)
  int32_t in_w, in_h;
  LensP lens;
  int32_t has_rot;
  int32_t in_vec;   // (launcher) four packed samples at a base aligned to them: one load per tap
  float rot[9];     // row-major; valid when has_rot
};

struct ComposePackedParams {
  // ---- what lrp_capi.cpp states ----
  void *dst;            // out_w x out_h pixels of out_channels samples in out_format
  uint8_t *count;       // the plane of k (out_w * out_h bytes, any alignment), or null
  int32_t out_w, out_h;
  int32_t channels;     // C: channels of the float images the chain would stage (<= kPackedMaxChannels)
  int32_t in_channels;  // packed samples per source texel, every source's
  int32_t out_channels; // packed samples per output pixel
  int32_t out_format;   // kPackedF32 / kPackedF16 / kPackedU8: a run-time switch
  uint32_t out_fill;    // the samples beyond C (the low 8 / 16 bits, or the bit pattern of a float)
  int32_t n_src;        // 1 .. kComposeMaxSources
  int32_t mode;         // kComposeFirst / kComposeMean / kComposeFeather
  int32_t has_post;     // fused post_process on the composed value
  float exposure, reinhard;
  LensP out_lens;
  // ---- what the launcher (lrp_compose_packed.hip) derives ----
  const float *decode, *threshold; // the device copy of the 8-bit tables (256 floats each)
  int32_t in_pitch, out_pitch;     // bytes per source texel / output pixel
  int32_t in_copy, out_copy;       // min(in_channels, C), min(C, out_channels): samples decoded / encoded; the rest is 0.0f / out_fill
  int32_t out_vec;                 // four packed samples at a base aligned to them: one store per pixel
  int32_t tiles_x, tiles_y;        // output tiling (lrp_kernel_impl.h: 32 x 8 pixels, xcd_tile numbering)
  ComposePackedSource src[kComposeMaxSources];
};

} // namespace lrp
