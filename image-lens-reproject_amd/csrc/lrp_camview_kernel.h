// lrp_camview_kernel.h — the camera-view kernel (include/lrp.h "calibrated camera as the target"): frames
// of calibrated cameras composed into the frame of another calibrated camera — a new camera matrix, camera-to-camera remapping,
// re-distortion — with n x n sub-samples per pixel, one launch.  Included by one unit per interpolation (lrp_camview.hip;
// lrp_camview_unit.hip twice, units.list) so that the three instantiation sets compile in parallel.
//
// Per output pixel: compose_ss_pixel (lrp_compose_pixel.h) with CameraSources (lrp_camera_kernel.h) and, in place of the target
// of an ideal lens, CameraTarget<TargetModel> below: camera_unproject (lrp_camera_inverse.h), the Newton inverse of the target's
// polynomial, which may find no ray.  A sub-sample without a ray is covered by no camera; the body compiles its has_ray tests
// for this target alone.  Nothing of the body is restated.
//
// Mapping (gfx950): lrp_compose_pixel.h's, the Newton loop among the wave-uniform loops that are not unrolled; and a ballot
// after the inverse, so that a wave none of whose lanes has a ray skips the source loop.  The target's model is a template
// parameter (one target per launch): 2 models x 3 samplers.  The sources' models stay a wave-uniform branch.
#pragma once

#include "lrp_camera_inverse.h"
#include "lrp_camera_kernel.h"
#include "lrp_camview.h"

namespace lrp {

using CameraViewKernelFn = void (*)(const CameraViewParams);

// A calibrated camera as the target (the Target policy of lrp_compose_pixel.h): sub-sample positions in pixels of the target
// (n == 1: the pixel's own x, y) and the Newton inverse.
template <int Model> struct CameraTarget {
  static constexpr bool kAlwaysRay = false;
  int x, y;
  template <typename Params> __device__ __forceinline__ CameraTarget(const Params &, int x_, int y_) : x(x_), y(y_) {}
  __device__ __forceinline__ float column(int ssx, float ns1) const { return ((float)x + ((float)ssx + 1.0f) / ns1) - 0.5f; }
  template <typename Params>
  __device__ __forceinline__ bool ray(const Params &P, float u, int ssy, float ns1, float &rx, float &ry, float &rz) const {
    const float v = ((float)y + ((float)ssy + 1.0f) / ns1) - 0.5f;
    return camera_unproject<Model>(P.target, u, v, rx, ry, rz);
  }
};

template <int TargetModel, int Interp>
__global__ __launch_bounds__(kComposeThreads) void camera_view_kernel(const CameraViewParams P) {
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;
  compose_ss_pixel<Interp, CameraSources, CameraTarget<TargetModel>>(P, x, y, NoSampleHook{});
}

template <int Interp> hipError_t launch_camera_view_interp(CameraViewParams P, hipStream_t stream) {
  CameraViewKernelFn fn = nullptr;
  if (P.target.model == kCameraBrown) fn = camera_view_kernel<kCameraBrown, Interp>;
  if (P.target.model == kCameraFisheye) fn = camera_view_kernel<kCameraFisheye, Interp>;
  return launch_compose_tiles(fn, P, P, stream);
}

// ... as a bilinear / bicubic unit of units.list compiles it: defined and instantiated by lrp_camview_unit.hip, declared only for the launcher.
template <int Interp> hipError_t launch_camera_view_unit(const CameraViewParams &P, hipStream_t stream);
} // namespace lrp
