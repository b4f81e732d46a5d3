// lrp_mb_packed.h — the argument block of the packed level-0 collapse of multi-band blending (lrp_mb_packed_kernel.h;
// include/lrp.h "multi-band blending, packed pixels"), shared by lrp_capi.cpp and lrp_mb_packed.hip.  The
// pyramid side is MultibandCollapseParams' at level 0 (lrp_multiband.h); the output side is CameraPackedParams' (lrp_camera_packed.h),
// field by field what store_packed (lrp_packed_kernel.h) reads.  A block of its own, so that the blocks — and with them the
// kernarg layout, the bytes and the time — of the calls that exist do not move.  Plain POD passed by value in kernarg:
// wave-uniform, scalar loads.
#pragma once

#include <stdint.h>

#include "lrp_multiband.h"
#include "lrp_packed.h"

namespace lrp {

struct MbCollapsePackedParams {
  // ---- what lrp_capi.cpp states ----
  const float *a;       // A_0, w x h x C
  const float *s;       // S_0, w x h
  const float *cr;      // R_1, cw x ch x C; not read when top
  void *dst;            // w x h pixels of out_channels samples in out_format, at any alignment
  const uint8_t *label; // kMultibandNoCamera pixels are +0.0f (code 0) in their first C channels
  int32_t w, h, cw, ch;
  int32_t wrap;
  int32_t top;          // num_bands == 0: R_0 = N_0
  int32_t has_post;
  float exposure, reinhard;
  int32_t out_channels; // packed samples per output pixel
  int32_t out_format;   // kPackedF32 / kPackedF16 / kPackedU8: a run-time switch
  uint32_t out_fill;    // the samples beyond C (the low 8 / 16 bits, or the bit pattern of a float)
  // ---- what the launcher (lrp_mb_packed.hip) derives ----
  const float *threshold; // the device copy of the 8-bit threshold table (256 floats)
  int32_t out_pitch;      // bytes per output pixel
  int32_t out_copy;       // min(C, out_channels): samples encoded; the rest is out_fill
  int32_t out_vec;        // four packed samples at a base aligned to them: one store per pixel
};

constexpr int mb_collapse_packed_lds_bytes(int channels) { return mb_expand_lds_bytes(channels) + 256 * 4; }

} // namespace lrp
