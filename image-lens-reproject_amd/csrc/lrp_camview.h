// lrp_camview.h — kernel argument block of the camera-view kernel (lrp_camview_kernel.h; include/lrp.h "calibrated camera as
// the target"), shared by lrp_capi.cpp and the lrp_camview*.hip units.  The fields of CameraParams
// (lrp_camera.h) with a camera descriptor in place of the ideal output lens; a block of its own, so that CameraParams — and with
// it the kernarg layout, the bytes and the time of lrp_compose_cameras_device — does not move.  Plain POD passed by value in
// kernarg: wave-uniform, read with scalar loads.
#pragma once

#include <stdint.h>

#include "lrp_camera.h"

namespace lrp {

struct CameraViewParams {
  float *dst;
  uint8_t *count;      // the plane of the number of cameras that cover at least one sub-sample, or null
  uint8_t *coverage;   // the plane of m, the number of covered sub-samples (0 .. n * n), or null
  int32_t out_w, out_h; // the target's width and height
  int32_t channels;    // floats per texel (the stride), every camera's and the output's
  int32_t ch_count;    // channels composed by this launch (<= kMaxDynChannels; dst and the cameras' data point at the first)
  int32_t n_src;       // 1 .. kComposeMaxSources
  int32_t mode;        // kComposeFirst / kComposeMean / kComposeFeather
  int32_t num_samples; // n: 1 .. kComposeSsMaxSamples sub-samples per axis
  int32_t has_post;    // fused post_process on the composed value
  float exposure, reinhard;
  int32_t tiles_x, tiles_y; // output tiling (lrp_kernel_impl.h: 32 x 8 pixels, xcd_tile numbering)
  CameraSource target; // fx, fy, cx, cy, k, limit; data, in_w, in_h, has_rot and rot are not read (the model is the kernel's)
  CameraSource src[kComposeMaxSources];
};

} // namespace lrp
