// lrp_camera_inverse.h — target pixel -> ray of a calibrated camera (include/lrp.h "calibrated camera as the target", DESIGN.md
// section 18): the inverse of the two distortion polynomials by a fixed number of Newton steps, in binary32, un-fused, in the
// order the header writes.  One function for the device (camera_view_kernel, lrp_camview_kernel.h) and for the host
// (lrp_camera_unproject, lrp_capi.cpp), so that both deliver the same bits; sqrt and sincos are lrp_math.h's, nothing of libm.
#pragma once

#include "lrp_camera.h"
#include "lrp_math.h"

namespace lrp {

constexpr int kCameraInverseSteps = 8; // LRP_CAMERA_INVERSE_STEPS

// Brown-Conrady forward map of the normalised point X, Y, and its residual against x0, y0 (the last evaluation of the
// definition; the loop below restates it because it shares r2, ab and L with the Jacobian).
LRP_HD void camera_brown_residual(const CameraSource &T, float X, float Y, float x0, float y0, float &ex, float &ey) {
  const float k1 = T.k[0], k2 = T.k[1], p1 = T.k[2], p2 = T.k[3], k3 = T.k[4];
  const float r2 = X * X + Y * Y;
  const float ab = X * Y;
  const float L = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
  const float xd = X * L + ((2.0f * p1) * ab + p2 * (r2 + 2.0f * (X * X)));
  const float yd = Y * L + (p1 * (r2 + 2.0f * (Y * Y)) + (2.0f * p2) * ab);
  ex = xd - x0;
  ey = yd - y0;
}

// The ray of target pixel position u, v (pixels; (0, 0) is the centre of the top-left texel) of camera T.  Returns has_ray; the
// ray is written either way (it may be NaN where has_ray is false).  The BROWN ray is (X, Y, -1), not normalised.
template <int Model> LRP_HD bool camera_unproject(const CameraSource &T, float u, float v, float &rx, float &ry, float &rz) {
  const float x0 = (u - T.cx) / T.fx;
  const float y0 = (v - T.cy) / T.fy;
  if (Model == kCameraFisheye) {
    const float k1 = T.k[0], k2 = T.k[1], k3 = T.k[2], k4 = T.k[3];
    const float rd = lrp_sqrtf(x0 * x0 + y0 * y0);
    float th = rd;
    bool ok = th <= T.limit;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int it = 0; it < kCameraInverseSteps; ++it) {
      const float t2 = th * th;
      const float g = th * (1.0f + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));
      const float gp = 1.0f + t2 * ((3.0f * k1) + t2 * ((5.0f * k2) + t2 * ((7.0f * k3) + t2 * (9.0f * k4))));
      th = th - (g - rd) / gp;
      ok = ok && th >= 0.0f && th <= T.limit; // sticky; NaN: false
    }
    const float t2 = th * th;
    const float g = th * (1.0f + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));
    const float e = g - rd;
    const bool has_ray = ok && lrp_fabsf(T.fx * e) <= 0.5f && lrp_fabsf(T.fy * e) <= 0.5f;
    float s, c;
    sincosf_(th, s, c);
    const float q = (rd > 0.0f) ? s / rd : 0.0f;
    rx = q * x0;
    ry = q * y0;
    rz = -c;
    return has_ray;
  }
  const float k1 = T.k[0], k2 = T.k[1], p1 = T.k[2], p2 = T.k[3], k3 = T.k[4];
  float X = x0, Y = y0;
  bool ok = X * X + Y * Y <= T.limit;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int it = 0; it < kCameraInverseSteps; ++it) {
    const float r2 = X * X + Y * Y;
    const float ab = X * Y;
    const float L = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
    const float D = k1 + r2 * ((2.0f * k2) + r2 * (3.0f * k3));
    const float xd = X * L + ((2.0f * p1) * ab + p2 * (r2 + 2.0f * (X * X)));
    const float yd = Y * L + (p1 * (r2 + 2.0f * (Y * Y)) + (2.0f * p2) * ab);
    const float ex = xd - x0;
    const float ey = yd - y0;
    const float jxx = ((L + (2.0f * (X * X)) * D) + (2.0f * p1) * Y) + (6.0f * p2) * X;
    const float jxy = (((2.0f * ab) * D) + (2.0f * p1) * X) + (2.0f * p2) * Y;
    const float jyy = ((L + (2.0f * (Y * Y)) * D) + (6.0f * p1) * Y) + (2.0f * p2) * X;
    const float det = jxx * jyy - jxy * jxy;
    const float Xn = X - (jyy * ex - jxy * ey) / det;
    const float Yn = Y - (jxx * ey - jxy * ex) / det;
    X = Xn;
    Y = Yn;
    ok = ok && (X * X + Y * Y <= T.limit); // sticky; NaN: false
  }
  float ex, ey;
  camera_brown_residual(T, X, Y, x0, y0, ex, ey);
  rx = X;
  ry = Y;
  rz = -1.0f;
  return ok && lrp_fabsf(T.fx * ex) <= 0.5f && lrp_fabsf(T.fy * ey) <= 0.5f;
}

} // namespace lrp
