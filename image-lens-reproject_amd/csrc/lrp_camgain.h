// lrp_camgain.h — kernel argument block of the calibrated-camera compose kernel with gains (lrp_camgain_kernel.h; include/lrp.h
// "exposure matching across a camera rig"), shared by lrp_capi.cpp and the lrp_camgain*.hip units.  The
// fields of CameraParams (lrp_camera.h) plus one gain per camera; a block of its own, so that CameraParams — and with it the
// kernarg layout, the bytes and the time of lrp_compose_cameras_device — does not move.  Plain POD passed by value in kernarg:
// wave-uniform, read with scalar loads.
#pragma once

#include "lrp_camera.h"

namespace lrp {

struct CameraGainParams {
  CameraParams cam;               // every field as lrp_compose_cameras_device fills it
  float gain[kComposeMaxSources]; // g_i: multiplies the first min(channels, 3) channels of camera i's sample
};

} // namespace lrp
