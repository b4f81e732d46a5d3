/*
 * camera_model.c — CPU model of compose with calibrated cameras (include/lrp.h "compose, calibrated cameras"; DESIGN.md
 * section 17): the definition written out per pixel.  The target lenses, the samplers and libm are those of
 * tests/native/coverage_model.c, included textually and unedited; the source mapping (Brown-Conrady, Kannala-Brandt) and its
 * coverage test are written here from the header's definition.  Test infrastructure.
 *
 * Build with the flags of coverage_model.c: -O3 -ffp-contract=off -fno-fast-math (no -march: no FMA).
 */
#include "coverage_model.c"

enum { CAM_BROWN = 0, CAM_FISHEYE = 1 };
enum { CAM_FIRST = 0, CAM_MEAN = 1, CAM_FEATHER = 2, CAM_MAX_SOURCES = 8, CAM_MAX_CHANNELS = 64 };

/* layout of include/lrp.h lrp_camera */
typedef struct {
  int32_t model;
  int32_t width, height;
  float *data;
  float fx, fy, cx, cy;
  float k[5];
  float limit;
} cam_camera;

static float cam_min(float a, float b) { return (b < a) ? b : a; }

/* ray -> source pixel; returns `imaged` */
static int cam_project(const cam_camera *S, float vx, float vy, float vz, float *sx, float *sy) {
  if (S->model == CAM_FISHEYE) {
    float k1 = S->k[0], k2 = S->k[1], k3 = S->k[2], k4 = S->k[3];
    float rho = sqrtf(vx * vx + vy * vy);
    float theta = atan2f(rho, -vz);
    float t2 = theta * theta;
    float td = theta * (1.0f + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))));
    float q = (rho > 0.0f) ? td / rho : 0.0f;
    *sx = S->fx * (q * vx) + S->cx;
    *sy = S->fy * (q * vy) + S->cy;
    return theta <= S->limit;
  }
  float k1 = S->k[0], k2 = S->k[1], p1 = S->k[2], p2 = S->k[3], k3 = S->k[4];
  float a = vx / -vz;
  float b = vy / -vz;
  float r2 = a * a + b * b;
  float ab = a * b;
  float L = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
  float xd = a * L + ((2.0f * p1) * ab + p2 * (r2 + 2.0f * (a * a)));
  float yd = b * L + (p1 * (r2 + 2.0f * (b * b)) + (2.0f * p2) * ab);
  *sx = S->fx * xd + S->cx;
  *sy = S->fy * yd + S->cy;
  return vz < 0.0f && r2 <= S->limit;
}

static int cam_covered(const cam_camera *S, int imaged, float sx, float sy) {
  return imaged && sx >= -0.5f && sx <= (float)S->width - 0.5f && sy >= -0.5f && sy <= (float)S->height - 0.5f;
}

/* n rays (x, y, z) -> sxy[n][2], imaged[n] */
void cam_project_rays(const cam_camera *S, const float *rays, int n, float *sxy, uint8_t *imaged) {
  for (int j = 0; j < n; ++j) imaged[j] = (uint8_t)cam_project(S, rays[3 * j], rays[3 * j + 1], rays[3 * j + 2], sxy + 2 * j, sxy + 2 * j + 1);
}

/* The rotated ray, the source pixel and the flags (bit 0 imaged, bit 1 covered) of every sub-sample of a num_samples = n call
 * of one camera: [height][width][n * n] in the loop's order (sub = n * ssx + ssy).  Any output may be NULL.  Returns 0 or -1. */
int cam_detail(const cam_camera *S, const cvm_image *out, int num_samples, const float *rm, float *ray, float *sxy, uint8_t *flags) {
  if (out->lens.type < 0 || out->lens.type > 4 || num_samples < 1 || num_samples > 15 || (S->model != CAM_BROWN && S->model != CAM_FISHEYE)) return -1;
  const int n = num_samples;
  ptrdiff_t at = 0;
  for (int y = 0; y < out->height; ++y) {
    for (int x = 0; x < out->width; ++x) {
      float cx = (x + 0.5f) - out->width * 0.5f;
      float cy = (y + 0.5f) - out->height * 0.5f;
      for (int ssx = 0; ssx < n; ++ssx) {
        float scx = cx + (ssx + 1.0f) / (n + 1.0f) - 0.5f;
        for (int ssy = 0; ssy < n; ++ssy, ++at) {
          float scy = cy + (ssy + 1.0f) / (n + 1.0f) - 0.5f;
          float v[3], sx, sy;
          target_ray(&out->lens, (float)out->width, (float)out->height, scx, scy, v);
          if (rm) {
            float nx = rm[0] * v[0] + rm[1] * v[1] + rm[2] * v[2];
            float ny = rm[3] * v[0] + rm[4] * v[1] + rm[5] * v[2];
            float nz = rm[6] * v[0] + rm[7] * v[1] + rm[8] * v[2];
            v[0] = nx, v[1] = ny, v[2] = nz;
          }
          int imaged = cam_project(S, v[0], v[1], v[2], &sx, &sy);
          if (ray) ray[3 * at] = v[0], ray[3 * at + 1] = v[1], ray[3 * at + 2] = v[2];
          if (sxy) sxy[2 * at] = sx, sxy[2 * at + 1] = sy;
          if (flags) flags[at] = (uint8_t)(imaged | (cam_covered(S, imaged, sx, sy) << 1));
        }
      }
    }
  }
  return 0;
}

/* cams: n_in cameras of out->channels channels; rotations: n_in x 9 or NULL; post: {exposure, reinhard} or NULL; count / coverage:
 * out->width * out->height bytes or NULL.  Returns 0, or -1 for an unknown lens / model / sampler / mode or a count out of range. */
int cam_compose(const cam_camera *cams, int n_in, const float *rotations, cvm_image *out, int num_samples, int interpolation, int mode,
                const float *post, uint8_t *count, uint8_t *coverage) {
  if (n_in < 1 || n_in > CAM_MAX_SOURCES || num_samples < 1 || num_samples > 15 || interpolation < 0 || interpolation > 2 || mode < 0 ||
      mode > 2 || out->channels < 1 || out->channels > CAM_MAX_CHANNELS || out->lens.type < 0 || out->lens.type > 4)
    return -1;
  cvm_image img[CAM_MAX_SOURCES] = {0}; /* the samplers' view of the cameras: size, channels and data */
  for (int i = 0; i < n_in; ++i) {
    if (cams[i].model != CAM_BROWN && cams[i].model != CAM_FISHEYE) return -1;
    img[i].width = cams[i].width, img[i].height = cams[i].height, img[i].channels = out->channels, img[i].data = cams[i].data;
  }
  const int n = num_samples, C = out->channels;
  float acc[CAM_MAX_CHANNELS], v[CAM_MAX_CHANNELS], s[CAM_MAX_CHANNELS];
  for (int y = 0; y < out->height; ++y) {
    for (int x = 0; x < out->width; ++x) {
      float cx = (x + 0.5f) - out->width * 0.5f;
      float cy = (y + 0.5f) - out->height * 0.5f;
      for (int c = 0; c < C; ++c) acc[c] = 0.0f;
      int m = 0;
      unsigned seen = 0;
      for (int ssx = 0; ssx < n; ++ssx) {
        float scx = cx + (ssx + 1.0f) / (n + 1.0f) - 0.5f;
        for (int ssy = 0; ssy < n; ++ssy) {
          float scy = cy + (ssy + 1.0f) / (n + 1.0f) - 0.5f;
          float r[3];
          target_ray(&out->lens, (float)out->width, (float)out->height, scx, scy, r);
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
      ptrdiff_t at = (ptrdiff_t)y * out->width + x;
      float *dst = out->data + at * C;
      if (m == 0) {
        for (int c = 0; c < C; ++c) dst[c] = 0.0f;
      } else {
        float rr = 1.0f / (float)m;
        for (int c = 0; c < C; ++c) dst[c] = acc[c] * rr;
        if (post) {
          float exposure = post[0], reinhard = post[1];
          for (int c = 0; c < (C < 3 ? C : 3); ++c) { /* post_process (src/reproject.cpp:421-437) */
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
