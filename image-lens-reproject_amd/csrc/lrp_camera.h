// lrp_camera.h — kernel argument block of the calibrated-camera compose kernel (lrp_camera_kernel.h; include/lrp.h
// "compose, calibrated cameras"), shared by lrp_capi.cpp and the lrp_camera*.hip units.  The fields of
// ComposeSsParams (lrp_compose_ss.h) with a camera descriptor in place of the ideal-lens source; a block of its own, so that
// ComposeSsParams — and with it the kernarg layout, the bytes and the time of lrp_compose_ss_device — does not move.  Plain POD
// passed by value in kernarg: wave-uniform, read with scalar loads.
#pragma once

#include <stdint.h>

#include "lrp_compose_ss.h"

namespace lrp {

enum : int { kCameraBrown = 0, kCameraFisheye = 1 }; // lrp_camera_model

// One calibrated camera: what the source mapping and sample<> read of it.  26 words, all scalar.
struct CameraSource {
  const float *data;
  int32_t in_w, in_h;
  int32_t model;   // kCameraBrown / kCameraFisheye
  int32_t has_rot;
  float fx, fy, cx, cy; // pixels; (0, 0) is the centre of the top-left texel
  float k[5];      // brown: k1 k2 p1 p2 k3; fisheye: k1 k2 k3 k4
  float limit;     // brown: largest r2 imaged; fisheye: largest theta
  float rot[9];    // row-major; valid when has_rot
};

struct CameraParams {
  float *dst;
  uint8_t *count;      // the plane of the number of cameras that cover at least one sub-sample, or null
  uint8_t *coverage;   // the plane of m, the number of covered sub-samples (0 .. n * n), or null
  int32_t out_w, out_h;
  int32_t channels;    // floats per texel (the stride), every camera's and the output's
  int32_t ch_count;    // channels composed by this launch (<= kMaxDynChannels; dst and the cameras' data point at the first)
  int32_t n_src;       // 1 .. kComposeMaxSources
  int32_t mode;        // kComposeFirst / kComposeMean / kComposeFeather
  int32_t num_samples; // n: 1 .. kComposeSsMaxSamples sub-samples per axis
  int32_t has_post;    // fused post_process on the composed value
  float exposure, reinhard;
  int32_t tiles_x, tiles_y; // output tiling (lrp_kernel_impl.h: 32 x 8 pixels, xcd_tile numbering)
  LensP out_lens;
  CameraSource src[kComposeMaxSources];
};

} // namespace lrp
