/*
 * camera_view_model.c — CPU model of compose into a calibrated target camera (include/lrp.h "calibrated camera as the target";
 * DESIGN.md section 18): the definition written out per pixel.  The source mapping, its coverage test, the samplers and libm
 * are those of tests/native/camera_model.c, included textually and unedited; the inverse from target pixel to ray is written
 * here from the header's definition.  Test infrastructure.
 *
 * Build with the flags of camera_model.c: -O3 -ffp-contract=off -fno-fast-math (no -march: no FMA).
 */
#include "camera_model.c"

enum { CAMVIEW_STEPS = 8 }; /* LRP_CAMERA_INVERSE_STEPS */

/* target pixel position u, v -> ray[3]; returns has_ray */
static int camview_ray(const cam_camera *T, float u, float v, float ray[3]) {
  float x0 = (u - T->cx) / T->fx;
  float y0 = (v - T->cy) / T->fy;
  if (T->model == CAM_FISHEYE) {
    float k1 = T->k[0], k2 = T->k[1], k3 = T->k[2], k4 = T->k[3];
    float rd = sqrtf(x0 * x0 + y0 * y0);
    float th = rd;
    int ok = th <= T->limit;
    for (int it = 0; it < CAMVIEW_STEPS; ++it) {
      float t2 = th * th;
      float g = th * (1.0f + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));
      float gp = 1.0f + t2 * ((3.0f * k1) + t2 * ((5.0f * k2) + t2 * ((7.0f * k3) + t2 * (9.0f * k4))));
      th = th - (g - rd) / gp;
      ok = ok && th >= 0.0f && th <= T->limit;
    }
    float t2 = th * th;
    float g = th * (1.0f + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));
    float e = g - rd;
    int has_ray = ok && fabsf(T->fx * e) <= 0.5f && fabsf(T->fy * e) <= 0.5f;
    float s = sinf(th), c = cosf(th);
    float q = (rd > 0.0f) ? s / rd : 0.0f;
    ray[0] = q * x0, ray[1] = q * y0, ray[2] = -c;
    return has_ray;
  }
  float k1 = T->k[0], k2 = T->k[1], p1 = T->k[2], p2 = T->k[3], k3 = T->k[4];
  float X = x0, Y = y0;
  int ok = X * X + Y * Y <= T->limit;
  for (int it = 0; it <= CAMVIEW_STEPS; ++it) { /* the last round evaluates xd, yd, ex, ey only */
    float r2 = X * X + Y * Y;
    float ab = X * Y;
    float L = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
    float xd = X * L + ((2.0f * p1) * ab + p2 * (r2 + 2.0f * (X * X)));
    float yd = Y * L + (p1 * (r2 + 2.0f * (Y * Y)) + (2.0f * p2) * ab);
    float ex = xd - x0, ey = yd - y0;
    if (it == CAMVIEW_STEPS) {
      ray[0] = X, ray[1] = Y, ray[2] = -1.0f;
      return ok && fabsf(T->fx * ex) <= 0.5f && fabsf(T->fy * ey) <= 0.5f;
    }
    float D = k1 + r2 * ((2.0f * k2) + r2 * (3.0f * k3));
    float jxx = ((L + (2.0f * (X * X)) * D) + (2.0f * p1) * Y) + (6.0f * p2) * X;
    float jxy = (((2.0f * ab) * D) + (2.0f * p1) * X) + (2.0f * p2) * Y;
    float jyy = ((L + (2.0f * (Y * Y)) * D) + (6.0f * p1) * Y) + (2.0f * p2) * X;
    float det = jxx * jyy - jxy * jxy;
    float Xn = X - (jyy * ex - jxy * ey) / det;
    float Yn = Y - (jxx * ey - jxy * ex) / det;
    X = Xn, Y = Yn;
    ok = ok && (X * X + Y * Y <= T->limit);
  }
  return 0; /* not reached */
}

static int camview_model_ok(const cam_camera *T) { return T->model == CAM_BROWN || T->model == CAM_FISHEYE; }

/* n positions uv[n][2] -> rays[n][3], has_ray[n] */
int camview_unproject(const cam_camera *T, const float *uv, int n, float *rays, uint8_t *has_ray) {
  if (!camview_model_ok(T)) return -1;
  for (int j = 0; j < n; ++j) has_ray[j] = (uint8_t)camview_ray(T, uv[2 * j], uv[2 * j + 1], rays + 3 * j);
  return 0;
}

static float camview_sub(int px, int ss, int n) { return ((float)px + ((float)ss + 1.0f) / ((float)n + 1.0f)) - 0.5f; }

/* The position, the ray and has_ray of every sub-sample of a num_samples = n call: [height][width][n * n] in the loop's order
 * (sub = n * ssx + ssy).  Any output may be NULL.  Returns 0 or -1. */
int camview_detail(const cam_camera *T, int num_samples, float *uv, float *ray, uint8_t *has_ray) {
  if (!camview_model_ok(T) || num_samples < 1 || num_samples > 15) return -1;
  const int n = num_samples;
  ptrdiff_t at = 0;
  for (int y = 0; y < T->height; ++y)
    for (int x = 0; x < T->width; ++x)
      for (int ssx = 0; ssx < n; ++ssx)
        for (int ssy = 0; ssy < n; ++ssy, ++at) {
          float u = camview_sub(x, ssx, n), v = camview_sub(y, ssy, n), r[3];
          int has = camview_ray(T, u, v, r);
          if (uv) uv[2 * at] = u, uv[2 * at + 1] = v;
          if (ray) ray[3 * at] = r[0], ray[3 * at + 1] = r[1], ray[3 * at + 2] = r[2];
          if (has_ray) has_ray[at] = (uint8_t)has;
        }
  return 0;
}

/* cams: n_in cameras of `channels` channels; rotations: n_in x 9 or NULL; target: its width and height are the output's, its
 * data is ignored; out: height * width * channels floats; post: {exposure, reinhard} or NULL; count / coverage: width * height
 * bytes or NULL.  Returns 0, or -1 for an unknown model / sampler / mode or a count out of range. */
int camview_compose(const cam_camera *cams, int n_in, const float *rotations, const cam_camera *T, float *out, int channels, int num_samples,
                    int interpolation, int mode, const float *post, uint8_t *count, uint8_t *coverage) {
  if (n_in < 1 || n_in > CAM_MAX_SOURCES || num_samples < 1 || num_samples > 15 || interpolation < 0 || interpolation > 2 || mode < 0 ||
      mode > 2 || channels < 1 || channels > CAM_MAX_CHANNELS || !camview_model_ok(T))
    return -1;
  cvm_image img[CAM_MAX_SOURCES] = {0}; /* the samplers' view of the cameras: size, channels and data */
  for (int i = 0; i < n_in; ++i) {
    if (!camview_model_ok(cams + i)) return -1;
    img[i].width = cams[i].width, img[i].height = cams[i].height, img[i].channels = channels, img[i].data = cams[i].data;
  }
  const int n = num_samples, C = channels;
  float acc[CAM_MAX_CHANNELS], v[CAM_MAX_CHANNELS], s[CAM_MAX_CHANNELS];
  for (int y = 0; y < T->height; ++y) {
    for (int x = 0; x < T->width; ++x) {
      for (int c = 0; c < C; ++c) acc[c] = 0.0f;
      int m = 0;
      unsigned seen = 0;
      for (int ssx = 0; ssx < n; ++ssx) {
        for (int ssy = 0; ssy < n; ++ssy) {
          float r[3];
          if (!camview_ray(T, camview_sub(x, ssx, n), camview_sub(y, ssy, n), r)) continue; /* no ray: no camera covers it */
          int k = 0;
          float wsum = 0.0f;
          for (int c = 0; c < C; ++c) v[c] = 0.0f;
          for (int i = 0; i < n_in; ++i) {
            const cam_camera *S = cams + i;
            float vx = r[0], vy = r[1], vz = r[2];
            if (rotations) {
              const float *rm = rotations + 9 * i;
              vx = rm[0] * r[0] + rm[1] * r[1] + rm[2] * r[2];
              vy = rm[3] * r[0] + rm[4] * r[1] + rm[5] * r[2];
              vz = rm[6] * r[0] + rm[7] * r[1] + rm[8] * r[2];
            }
            float sx, sy;
            int imaged = cam_project(S, vx, vy, vz, &sx, &sy);
            if (!cam_covered(S, imaged, sx, sy)) continue;
            seen |= 1u << i;
            ++k;
            if (mode == CAM_FIRST && k > 1) continue;
            if (interpolation == 0)
              tap_nearest(img + i, 0, sx, sy, s);
            else if (interpolation == 1)
              tap_bilinear(img + i, 0, sx, sy, s);
            else
              tap_bicubic(img + i, 0, sx, sy, s);
            if (mode == CAM_FIRST) {
              for (int c = 0; c < C; ++c) v[c] = s[c];
            } else if (mode == CAM_MEAN) {
              for (int c = 0; c < C; ++c) v[c] = v[c] + s[c];
            } else {
              float dy = cam_min(sy + 0.5f, ((float)S->height - 0.5f) - sy);
              float d = cam_min(cam_min(sx + 0.5f, ((float)S->width - 0.5f) - sx), dy);
              float w = (d < 0x1p-10f) ? 0x1p-10f : d;
              for (int c = 0; c < C; ++c) {
                float t = w * s[c];
                v[c] = v[c] + t;
              }
              wsum = wsum + w;
            }
          }
          if (k == 0) continue;
          if (mode != CAM_FIRST) {
            float div = mode == CAM_MEAN ? (float)k : wsum;
            for (int c = 0; c < C; ++c) v[c] = v[c] / div;
          }
          for (int c = 0; c < C; ++c) acc[c] = acc[c] + v[c];
          ++m;
        }
      }
      ptrdiff_t at = (ptrdiff_t)y * T->width + x;
      float *dst = out + at * C;
      if (m == 0) {
        for (int c = 0; c < C; ++c) dst[c] = 0.0f;
      } else {
        float rr = 1.0f / (float)m;
        for (int c = 0; c < C; ++c) dst[c] = acc[c] * rr;
        if (post) {
          float exposure = post[0], reinhard = post[1];
          for (int c = 0; c < (C < 3 ? C : 3); ++c) { /* post_process, as camera_model.c writes it */
            float t = dst[c];
            t *= exposure;
            t = t * (1.0f + t / (reinhard * reinhard)) / (1.0f + t);
            dst[c] = t;
          }
        }
      }
      if (count) count[at] = (uint8_t)__builtin_popcount(seen);
      if (coverage) coverage[at] = (uint8_t)m;
    }
  }
  return 0;
}
