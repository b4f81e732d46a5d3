// lrp_camera_kernel.h — the calibrated-camera compose kernel (include/lrp.h "compose, calibrated cameras", DESIGN.md section
// 17): several frames of calibrated cameras — fx, fy, cx, cy in pixels plus Brown-Conrady or Kannala-Brandt coefficients —
// into one output with n x n sub-samples per pixel, one launch.  Included by one unit per interpolation (lrp_camera.hip;
// lrp_camera_unit.hip twice, units.list) so that the three instantiation sets compile in parallel.
//
// Per output pixel: compose_ss_pixel (lrp_compose_pixel.h), the supersampled body, with CameraSources below in place of the
// sources of an ideal lens: camera_project, the closed-form polynomial from ray to source pixel, its `imaged` test and the box
// test.  The target stays IdealTarget<OutLens>; there is no per-sample hook.  Nothing of the body is restated; atan2f_ is
// lrp_math.h's.
//
// Mapping (gfx950): lrp_compose_pixel.h's; a camera's descriptor is nine rotation floats and twelve camera floats of scalar
// loads, none of which occupies a VGPR across the loop.  The camera model is a wave-uniform branch on an SGPR, not a template
// parameter: rigs may mix models, and the instantiations stay at 5 output lenses x 3 samplers.
#pragma once

#include "lrp_camera.h"
#include "lrp_compose_pixel.h"

namespace lrp {

using CameraKernelFn = void (*)(const CameraParams);

// Ray -> source pixel of camera S (include/lrp.h "compose, calibrated cameras"): binary32, un-fused, in the order written
// there.  Returns `imaged`.
__device__ __forceinline__ bool camera_project(const CameraSource &S, float vx, float vy, float vz, float &sx, float &sy) {
  if (S.model == kCameraFisheye) { // wave-uniform
    const float rho = lrp_sqrtf(vx * vx + vy * vy);
    const float theta = atan2f_(rho, -vz);
    const float t2 = theta * theta;
    const float td = theta * (1.0f + t2 * (S.k[0] + t2 * (S.k[1] + t2 * (S.k[2] + t2 * S.k[3]))));
    const float q = (rho > 0.0f) ? td / rho : 0.0f;
    sx = S.fx * (q * vx) + S.cx;
    sy = S.fy * (q * vy) + S.cy;
    return theta <= S.limit;
  }
  const float k1 = S.k[0], k2 = S.k[1], p1 = S.k[2], p2 = S.k[3], k3 = S.k[4];
  const float a = vx / -vz;
  const float b = vy / -vz;
  const float r2 = a * a + b * b;
  const float ab = a * b;
  const float L = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
  const float xd = a * L + ((2.0f * p1) * ab + p2 * (r2 + 2.0f * (a * a)));
  const float yd = b * L + (p1 * (r2 + 2.0f * (b * b)) + (2.0f * p2) * ab);
  sx = S.fx * xd + S.cx;
  sy = S.fy * yd + S.cy;
  return vz < 0.0f && r2 <= S.limit;
}

// Calibrated cameras as the sources (the Sources policy of lrp_compose_pixel.h).
struct CameraSources {
  static constexpr bool kLoop = false;
  static __device__ __forceinline__ bool map(const CameraSource &S, float vx, float vy, float vz, float in_w, float in_h, float &sx, float &sy) {
    const bool imaged = camera_project(S, vx, vy, vz, sx, sy);
    // covered iff imaged && in_x && in_y; comparisons with NaN are false
    return imaged && sx >= -0.5f && sx <= in_w - 0.5f && sy >= -0.5f && sy <= in_h - 0.5f;
  }
};

template <int OutLens, int Interp>
__global__ __launch_bounds__(kComposeThreads) void compose_cam_kernel(const CameraParams P) {
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;
  compose_ss_pixel<Interp, CameraSources, IdealTarget<OutLens>>(P, x, y, NoSampleHook{});
}

// The kernels: one per output lens id (0 .. kLensIds - 1; the extension lenses are gated by the caller's validation).
template <int Interp, int... OutLens>
constexpr std::array<CameraKernelFn, kLensIds> camera_kernel_table(std::integer_sequence<int, OutLens...>) {
  return {{compose_cam_kernel<OutLens, Interp>...}};
}
// The kernel of output lens out_lens; nullptr: no such lens.
template <int Interp> CameraKernelFn camera_kernel(int out_lens) {
  static_assert(is_lens_id(0) && is_lens_id(kLensIds - 1), "every id 0 .. kLensIds - 1 names a lens");
  static constexpr std::array<CameraKernelFn, kLensIds> table = camera_kernel_table<Interp>(std::make_integer_sequence<int, kLensIds>{});
  if (out_lens < 0 || out_lens >= kLensIds) return nullptr;
  return table[out_lens];
}

template <int Interp> hipError_t launch_compose_cameras_interp(CameraParams P, int out_lens, hipStream_t stream) {
  return launch_compose_tiles(camera_kernel<Interp>(out_lens), P, P, stream);
}

// ... as a bilinear / bicubic unit of units.list compiles it: defined and instantiated by lrp_camera_unit.hip, declared only for the launcher.
template <int Interp> hipError_t launch_compose_cameras_unit(const CameraParams &P, int out_lens, hipStream_t stream);
} // namespace lrp
