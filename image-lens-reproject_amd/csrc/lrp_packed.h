// lrp_packed.h — kernel argument block of the packed-pixel kernel (lrp_packed_kernel.h; include/lrp.h "packed pixels", DESIGN.md
// section 13), shared by lrp_capi.cpp and the lrp_packed*.hip units.  Plain POD passed by value in kernarg like KParams
// (lrp_params.h): wave-uniform, read with scalar loads.
#pragma once

#include <stdint.h>

#include "lrp_params.h"

namespace lrp {

enum : int { kPackedF32 = 0, kPackedF16 = 1, kPackedU8 = 2 }; // lrp_pixel_format
constexpr int kPackedMaxChannels = 8;                         // the run-time channel path of lrp_device.h (kMaxDynChannels)

struct PackedParams {
  // ---- what lrp_capi.cpp states ----
  const void *src; // in_w x in_h texels of in_channels packed samples (binary16 or 8-bit; the format is a template argument)
  void *dst;       // out_w x out_h pixels of out_channels samples in out_format
  int32_t in_w, in_h;
  int32_t out_w, out_h;
  int32_t channels;     // C: channels of the float image the chain would stage (<= kPackedMaxChannels)
  int32_t in_channels;  // packed samples per source texel
  int32_t out_channels; // packed samples per output pixel
  int32_t out_format;   // kPackedF32 / kPackedF16 / kPackedU8: a run-time switch
  uint32_t out_fill;    // the samples beyond C (the low 8 / 16 bits, or the bit pattern of a float)
  int32_t num_samples;
  float normalize;      // 1.0f / (num_samples * num_samples), src/reproject.cpp:280
  LensP in_lens, out_lens;
  float rot[9];         // row-major; valid when has_rot
  int32_t has_rot;
  int32_t has_post;     // fused post_process (src/reproject.cpp:421-437)
  float exposure, reinhard;
  int32_t geo_mode;     // geometry cache (lrp_geocache.h): 0 compute, 1 compute and write geo_xy, 2 read geo_xy (the GeoRead kernels)
  float *geo_xy;        // (sx, sy) per output pixel, element geo_map_index(x, y) (lrp_params.h)
  // ---- what the launcher (lrp_packed.hip) derives ----
  const float *decode, *threshold; // the device copy of the 8-bit tables (256 floats each)
  int32_t in_pitch, out_pitch;     // bytes per source texel / output pixel
  int32_t in_copy, out_copy;       // min(in_channels, C), min(C, out_channels): samples decoded / encoded; the rest is 0.0f / out_fill
  int32_t in_vec, out_vec;         // four packed samples at a base aligned to them: one load / store per texel
  int32_t tiles_x, tiles_y;        // output tiling (lrp_kernel_impl.h: 32 x 8 pixels, xcd_tile numbering)
};

} // namespace lrp
