/*
 * coverage_model.c — CPU model of the coverage planes (include/lrp.h "coverage").  Derived from
 * tests/native/stereographic_model.c: the same loop, samplers and five lenses (its render is pinned to that model bit for bit by
 * tests/test_coverage.py, so the lens code is the proven one), plus cvm_coverage(), which calls the very lens functions the
 * render loop calls — cvm_source_ray() is cvm_source_position() with the rotated ray's z handed out — and applies the
 * definition per sub-sample.  Test infrastructure.
 *
 * Build with the oracle's float flags: -O3 -ffp-contract=off -fno-fast-math (no -march: no FMA).
 */
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

enum { CVM_RECT = 0, CVM_EQUIDISTANT = 1, CVM_EQUISOLID = 2, CVM_STEREOGRAPHIC = 3, CVM_EQUIRECT = 4 };

/* layouts of include/lrp.h lrp_lens / lrp_image */
typedef struct {
  int32_t type;
  float u[4]; /* rectilinear {focal}; equidistant {fov}; equisolid {focal, fov}; stereographic {focal}; equirect {lat_min, lat_max, lon_min, lon_max} */
  float sensor_width, sensor_height;
} cvm_lens;
typedef struct {
  cvm_lens lens;
  int32_t width, height, channels;
  float *data;
  int32_t data_layout;
} cvm_image;

static int trunc_x86(float v) {
  if (!(fabsf(v) < 2147483648.0f)) return INT_MIN;
  return (int)v;
}
static int clamp_index(int x, int lo, int hi) {
  int m = (hi < x) ? hi : x;
  return (lo < m) ? m : lo;
}
static int wrap_index(int i, int w) {
  int t = (int)((unsigned)i + (unsigned)w);
  int r = t % w;
  return (r < 0) ? 0 : r;
}
static float unit_clamp(float v) {
  float m = (v < 1.0f) ? v : 1.0f;
  return (0.0f < m) ? m : 0.0f;
}

/* ---- the equisolid lens (include/lrp.h) ---- */
static void cvm_equisolid_to_vec(const cvm_lens *L, float img_w, float cx, float cy, float v[3]) {
  float r_px = sqrtf(cx * cx + cy * cy);
  float r_mm = r_px / img_w * L->sensor_width;
  float theta = 2.0f * asinf(r_mm / (2.0f * L->u[0]));
  float s = sinf(theta) / r_px;
  v[0] = s * cx;
  v[1] = s * cy;
  v[2] = cosf(theta);
}
static void cvm_vec_to_equisolid(const cvm_lens *L, float img_w, float x, float y, float z, float *cx, float *cy) {
  x = x / -z;
  y = y / -z;
  float r = sqrtf(x * x + y * y);
  float theta = atanf(r);
  float r_mm = (2.0f * L->u[0]) * sinf(0.5f * theta);
  float r_px = r_mm / L->sensor_width * img_w;
  *cx = x / r * r_px;
  *cy = y / r * r_px;
}

/* ---- the stereographic lens (include/lrp.h): no libm call but sqrtf ---- */
static void cvm_stereographic_to_vec(const cvm_lens *L, float img_w, float cx, float cy, float v[3]) {
  float F = 2.0f * L->u[0];
  float r_px = sqrtf(cx * cx + cy * cy);
  float r_mm = r_px / img_w * L->sensor_width;
  float t = r_mm / F;
  float t2 = t * t;
  float d = 1.0f + t2;
  float s = ((2.0f * t) / d) / r_px;
  v[0] = s * cx;
  v[1] = s * cy;
  v[2] = (1.0f - t2) / d;
}
static void cvm_vec_to_stereographic(const cvm_lens *L, float img_w, float x, float y, float z, float *cx, float *cy) {
  float F = 2.0f * L->u[0];
  x = x / -z;
  y = y / -z;
  float r = sqrtf(x * x + y * y);
  float t = r / (1.0f + sqrtf(1.0f + r * r));
  float r_mm = F * t;
  float r_px = r_mm / L->sensor_width * img_w;
  *cx = x / r * r_px;
  *cy = y / r * r_px;
}

static void target_ray(const cvm_lens *L, float img_w, float img_h, float cx, float cy, float v[3]) {
  switch (L->type) {
  case CVM_RECT: {
    float focal = L->u[0];
    v[0] = cx / img_w * L->sensor_width / focal;
    v[1] = cy / img_h * L->sensor_height / focal;
    v[2] = -1.0f;
    break;
  }
  case CVM_EQUIDISTANT: {
    float fov = L->u[0];
    float r_px = sqrtf(cx * cx + cy * cy);
    float r_mm = r_px / img_w * L->sensor_width;
    float focal = L->sensor_width / fov;
    float theta = r_mm / focal;
    float s = sinf(theta) / r_px;
    v[0] = s * cx;
    v[1] = s * cy;
    v[2] = cosf(theta);
    break;
  }
  case CVM_EQUISOLID:
    cvm_equisolid_to_vec(L, img_w, cx, cy, v);
    break;
  case CVM_STEREOGRAPHIC:
    cvm_stereographic_to_vec(L, img_w, cx, cy, v);
    break;
  default: {
    float lat_min = L->u[0], lat_max = L->u[1], lon_min = L->u[2], lon_max = L->u[3];
    float lon_span = lon_max - lon_min;
    float lat_span = lat_max - lat_min;
    float lon = ((cx / img_w) + 0.5f) * lon_span + lon_min;
    float lat = ((cy / img_h) + 0.5f) * lat_span + lat_min;
    v[0] = sinf(lon);
    v[2] = -cosf(lon);
    v[1] = sinf(lat);
    break;
  }
  }
}

static void ray_to_source(const cvm_lens *L, float img_w, float img_h, float x, float y, float z, float *cx, float *cy) {
  switch (L->type) {
  case CVM_RECT: {
    float focal = L->u[0];
    x /= -z;
    y /= -z;
    *cx = x * img_w / L->sensor_width * focal;
    *cy = y * img_h / L->sensor_height * focal;
    break;
  }
  case CVM_EQUIDISTANT: {
    float fov = L->u[0];
    x /= -z;
    y /= -z;
    float r = sqrtf(x * x + y * y);
    float theta = atanf(r);
    float focal = L->sensor_width / fov;
    float r_mm = focal * theta;
    float r_px = r_mm / L->sensor_width * img_w;
    *cx = x / r * r_px;
    *cy = y / r * r_px;
    break;
  }
  case CVM_EQUISOLID:
    cvm_vec_to_equisolid(L, img_w, x, y, z, cx, cy);
    break;
  case CVM_STEREOGRAPHIC:
    cvm_vec_to_stereographic(L, img_w, x, y, z, cx, cy);
    break;
  default: {
    float lat_min = L->u[0], lat_max = L->u[1], lon_min = L->u[2], lon_max = L->u[3];
    float theta = -atan2f(-x, -z);
    float phi = asinf(y / sqrtf(x * x + y * y + z * z));
    float lon_span = lon_max - lon_min;
    float lat_span = lat_max - lat_min;
    *cx = ((theta - lon_min) / lon_span - 0.5f) * img_w;
    *cy = ((phi - lat_min) / lat_span - 0.5f) * img_h;
    break;
  }
  }
}

static int column(int i, int w, int loop) { return loop ? wrap_index(i, w) : clamp_index(i, 0, w - 1); }

static void tap_nearest(const cvm_image *img, int loop, float sx, float sy, float *out) {
  int lx = column(trunc_x86(sx + 0.5f), img->width, loop);
  int ly = clamp_index(trunc_x86(sy + 0.5f), 0, img->height - 1);
  const float *src = img->data + ((ptrdiff_t)ly * img->width + lx) * img->channels;
  for (int c = 0; c < img->channels; ++c) out[c] = src[c];
}

static void tap_bilinear(const cvm_image *img, int loop, float sx, float sy, float *out) {
  int w = img->width, h = img->height, C = img->channels;
  int lx = column(trunc_x86(sx), w, loop);
  int ux = column(trunc_x86(sx + 1.0f), w, loop);
  int ly = clamp_index(trunc_x86(sy), 0, h - 1);
  int uy = clamp_index(trunc_x86(sy + 1.0f), 0, h - 1);
  float fx = unit_clamp(sx - (float)lx), fy = unit_clamp(sy - (float)ly);
  float cfx = 1.0f - fx, cfy = 1.0f - fy;
  const float *row_l = img->data + (ptrdiff_t)ly * w * C, *row_u = img->data + (ptrdiff_t)uy * w * C;
  for (int c = 0; c < C; ++c) {
    float lo = fx * row_l[ux * C + c] + cfx * row_l[lx * C + c];
    float hi = fx * row_u[ux * C + c] + cfx * row_u[lx * C + c];
    out[c] = fy * hi + cfy * lo;
  }
}

static float catmull_rom(float a, float b, float c, float d, float t) {
  float inner = ((3.0f * (b - c)) + d) - a;
  float mid = ((((2.0f * a) - (5.0f * b)) + (4.0f * c)) - d) + t * inner;
  float outer = (c - a) + t * mid;
  return b + (0.5f * t) * outer;
}

static void tap_bicubic(const cvm_image *img, int loop, float sx, float sy, float *out) {
  int w = img->width, h = img->height, C = img->channels;
  int xs[4], ys[4];
  for (int k = 0; k < 4; ++k) {
    xs[k] = column(trunc_x86(sx + (float)(k - 1)), w, loop);
    ys[k] = clamp_index(trunc_x86(sy + (float)(k - 1)), 0, h - 1);
  }
  float fx = unit_clamp(sx - (float)xs[1]), fy = unit_clamp(sy - (float)ys[1]);
  ptrdiff_t pitch = (ptrdiff_t)w * C;
  for (int c = 0; c < C; ++c) {
    float col[4];
    for (int i = 0; i < 4; ++i) {
      const float *p = img->data + (ptrdiff_t)xs[i] * C + c;
      col[i] = catmull_rom(p[ys[0] * pitch], p[ys[1] * pitch], p[ys[2] * pitch], p[ys[3] * pitch], fy);
    }
    out[c] = catmull_rom(col[0], col[1], col[2], col[3], fx);
  }
}

static int source_wraps(const cvm_lens *L) {
  if (L->type != CVM_EQUIRECT) return 0;
  float long_range = L->u[3] - L->u[2];
  return fabs((double)long_range - (2 * M_PI)) < 1e-5f;
}

/* top-left-origin source texel coordinates of one sub-sample, and the z of its ray after the optional rotation */
void cvm_source_ray(const cvm_image *in, const cvm_image *out, const float *rm, float scx, float scy, float *sx, float *sy, float *vz) {
  float v[3];
  target_ray(&out->lens, (float)out->width, (float)out->height, scx, scy, v);
  if (rm) {
    float nx = rm[0] * v[0] + rm[1] * v[1] + rm[2] * v[2];
    float ny = rm[3] * v[0] + rm[4] * v[1] + rm[5] * v[2];
    float nz = rm[6] * v[0] + rm[7] * v[1] + rm[8] * v[2];
    v[0] = nx;
    v[1] = ny;
    v[2] = nz;
  }
  float px, py;
  ray_to_source(&in->lens, (float)in->width, (float)in->height, v[0], v[1], v[2], &px, &py);
  *sx = (px - 0.5f) + in->width * 0.5f;
  *sy = (py - 0.5f) + in->height * 0.5f;
  *vz = v[2];
}
void cvm_source_position(const cvm_image *in, const cvm_image *out, const float *rm, float scx, float scy, float *sx, float *sy) {
  float vz;
  cvm_source_ray(in, out, rm, scx, scy, sx, sy, &vz);
}

/* the definition of include/lrp.h for one sub-sample */
static int covered(const cvm_image *in, int loop, float sx, float sy, float vz) {
  int front = in->lens.type == CVM_EQUIRECT ? 1 : vz < 0.0f;
  int in_x = loop ? sx == sx : (sx >= -0.5f && sx <= (float)in->width - 0.5f);
  int in_y = sy >= -0.5f && sy <= (float)in->height - 0.5f;
  return front && in_x && in_y;
}

/* The count plane (one byte per output pixel, row-major) of a num_samples = n call, n <= 15; sxy / vz (may be NULL): the
 * coordinates and the rotated z of every sub-sample, [height][width][n * n] in the loop's order (sub = n * ssx + ssy).
 * Returns 0, or -1 for an unknown lens / n out of range. */
int cvm_coverage(const cvm_image *in, const cvm_image *out, int num_samples, const float *rotation, uint8_t *plane, float *sxy, float *vz_out) {
  const int types_ok = in->lens.type >= 0 && in->lens.type <= 4 && out->lens.type >= 0 && out->lens.type <= 4;
  if (!types_ok || num_samples < 1 || num_samples > 15) return -1;
  const int loop = source_wraps(&in->lens), n2 = num_samples * num_samples;
  for (int y = 0; y < out->height; ++y) {
    for (int x = 0; x < out->width; ++x) {
      float cx = (x + 0.5f) - out->width * 0.5f;
      float cy = (y + 0.5f) - out->height * 0.5f;
      int count = 0;
      ptrdiff_t at = ((ptrdiff_t)y * out->width + x) * n2;
      for (int ssx = 0; ssx < num_samples; ++ssx) {
        float scx = cx + (ssx + 1.0f) / (num_samples + 1.0f) - 0.5f;
        for (int ssy = 0; ssy < num_samples; ++ssy, ++at) {
          float scy = cy + (ssy + 1.0f) / (num_samples + 1.0f) - 0.5f;
          float sx, sy, vz;
          cvm_source_ray(in, out, rotation, scx, scy, &sx, &sy, &vz);
          count += covered(in, loop, sx, sy, vz);
          if (sxy) sxy[2 * at] = sx, sxy[2 * at + 1] = sy;
          if (vz_out) vz_out[at] = vz;
        }
      }
      plane[(ptrdiff_t)y * out->width + x] = (uint8_t)count;
    }
  }
  return 0;
}

/* the reference loop (src/reproject.cpp:280-341) over output rows [y_begin, y_end) (rows are independent); channels <= 64.
 * Returns 0, or -1 for an unknown lens / sampler. */
int cvm_reproject_rows(const cvm_image *in, cvm_image *out, int num_samples, int interpolation, const float *rotation, int y_begin,
                       int y_end) {
  const int types_ok = in->lens.type >= 0 && in->lens.type <= 4 && out->lens.type >= 0 && out->lens.type <= 4;
  if (!types_ok || interpolation < 0 || interpolation > 2 || out->channels > 64) return -1;
  const int loop = source_wraps(&in->lens), C = out->channels;
  const float normalize = 1.0f / (num_samples * num_samples);
  float acc[64], tap[64];
  if (y_begin < 0) y_begin = 0;
  if (y_end > out->height) y_end = out->height;
  for (int y = y_begin; y < y_end; ++y) {
    for (int x = 0; x < out->width; ++x) {
      float cx = (x + 0.5f) - out->width * 0.5f;
      float cy = (y + 0.5f) - out->height * 0.5f;
      for (int c = 0; c < C; ++c) acc[c] = 0.0f;
      for (int ssx = 0; ssx < num_samples; ++ssx) {
        float scx = cx + (ssx + 1.0f) / (num_samples + 1.0f) - 0.5f;
        for (int ssy = 0; ssy < num_samples; ++ssy) {
          float scy = cy + (ssy + 1.0f) / (num_samples + 1.0f) - 0.5f;
          float sx, sy;
          cvm_source_position(in, out, rotation, scx, scy, &sx, &sy);
          if (interpolation == 0)
            tap_nearest(in, loop, sx, sy, tap);
          else if (interpolation == 1)
            tap_bilinear(in, loop, sx, sy, tap);
          else
            tap_bicubic(in, loop, sx, sy, tap);
          for (int c = 0; c < C; ++c) acc[c] += tap[c];
        }
        float *dst = out->data + ((ptrdiff_t)y * out->width + x) * C;
        for (int c = 0; c < C; ++c) dst[c] = acc[c] * normalize;
      }
    }
  }
  return 0;
}

int cvm_reproject(const cvm_image *in, cvm_image *out, int num_samples, int interpolation, const float *rotation) {
  return cvm_reproject_rows(in, out, num_samples, interpolation, rotation, 0, out->height);
}

/* post_process (src/reproject.cpp:421-437) */
void cvm_post_process(cvm_image *img, float exposure, float reinhard) {
  int ch = img->channels < 3 ? img->channels : 3;
  ptrdiff_t n = (ptrdiff_t)img->width * img->height;
  float *p = img->data;
  for (ptrdiff_t i = 0; i < n; ++i, p += img->channels)
    for (int c = 0; c < ch; ++c) {
      float v = p[c];
      v *= exposure;
      v = v * (1.0f + v / (reinhard * reinhard)) / (1.0f + v);
      p[c] = v;
    }
}
