// lrp_camera_packed.h — kernel argument blocks of the packed camera kernels (lrp_camera_packed_kernel.h,
// lrp_camstat_packed_kernel.h; include/lrp.h "calibrated cameras, packed pixels"), shared by lrp_capi.cpp
// and the lrp_camera_packed*.hip / lrp_camstat_packed.hip units.  The camera descriptors are lrp_camera.h's CameraSource, whose
// `data` carries the pointer to packed samples; the output side is ComposePackedParams' (lrp_compose_packed.h), field by field
// what store_packed (lrp_packed_kernel.h) reads.  Blocks of their own, so that the blocks — and with them the kernarg layout, the
// bytes and the time — of the calls that exist do not move.  Plain POD passed by value in kernarg: wave-uniform, scalar loads.
#pragma once

#include <stdint.h>

#include "lrp_camera.h"
#include "lrp_camstat.h"
#include "lrp_packed.h"

namespace lrp {

struct CameraPackedParams {
  // ---- what lrp_capi.cpp states ----
  void *dst;            // out_w x out_h pixels of out_channels samples in out_format
  uint8_t *count;       // the plane of the number of cameras that cover at least one sub-sample, or null
  uint8_t *coverage;    // the plane of m, the number of covered sub-samples (0 .. n * n), or null
  int32_t out_w, out_h;
  int32_t channels;     // C: channels of the float images the chain would stage (<= kPackedMaxChannels)
  int32_t in_channels;  // packed samples per camera texel, every camera's
  int32_t out_channels; // packed samples per output pixel
  int32_t out_format;   // kPackedF32 / kPackedF16 / kPackedU8: a run-time switch
  uint32_t out_fill;    // the samples beyond C (the low 8 / 16 bits, or the bit pattern of a float)
  int32_t n_src;        // 1 .. kComposeMaxSources
  int32_t mode;         // kComposeFirst / kComposeMean / kComposeFeather
  int32_t num_samples;  // n: 1 .. kComposeSsMaxSamples sub-samples per axis
  int32_t has_post;     // fused post_process on the composed value
  float exposure, reinhard;
  LensP out_lens;
  float gain[kComposeMaxSources]; // g_i on the first min(C, 3) channels of camera i's decoded sample; 1.0f: a call without gains
  // ---- what the launcher (lrp_camera_packed.hip) derives ----
  const float *decode, *threshold; // the device copy of the 8-bit tables (256 floats each)
  int32_t in_pitch, out_pitch;     // bytes per camera texel / output pixel
  int32_t in_copy, out_copy;       // min(in_channels, C), min(C, out_channels): samples decoded / encoded; the rest is 0.0f / out_fill
  uint32_t in_vec;                 // bit i: camera i holds four packed samples at a base aligned to them — one load per tap
  int32_t out_vec;                 // four packed samples at a base aligned to them: one store per pixel
  int32_t tiles_x, tiles_y;        // output tiling (32 x 8 pixels, xcd_tile numbering)
  CameraSource src[kComposeMaxSources];
};

struct CameraStatPackedParams {
  // ---- what lrp_capi.cpp states ----
  unsigned long long *stats; // kOverlapWords words, zeroed ahead of the launch
  int32_t out_w, out_h;
  int32_t channels;          // C: channels of the float frames the chain would stage
  int32_t in_channels;       // packed samples per camera texel
  int32_t n_src;             // 1 .. kComposeMaxSources
  float lo, hi;              // 0 <= lo <= hi <= 32768
  LensP out_lens;
  // ---- what the launcher (lrp_camstat_packed.hip) derives ----
  const float *decode;       // the device copy of the 8-bit decode table
  int32_t ch_count;          // min(C, 3): the channels the luminance reads
  int32_t in_pitch;          // bytes per camera texel
  int32_t in_copy;           // min(in_channels, ch_count): samples decoded; the rest is 0.0f
  uint32_t in_vec;           // bit i: as CameraPackedParams::in_vec
  int32_t tiles_x, tiles_y;  // output tiling (32 x 8 pixels, xcd_tile numbering)
  int32_t n_groups;          // workgroup numbers of the tiling: kXcds * xcd_rows(tiles_y) * tiles_x
  CameraSource src[kComposeMaxSources];
};

} // namespace lrp
