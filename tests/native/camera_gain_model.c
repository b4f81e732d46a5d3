/*
 * camera_gain_model.c — CPU model of exposure matching across a camera rig (include/lrp.h "exposure matching across a camera
 * rig"): the overlap statistic and compose with one gain per camera, both written out per pixel from the
 * header's definition.  The target lenses, the samplers, libm and the camera polynomials are those of
 * tests/native/camera_model.c, included textually and unedited.  Test infrastructure.
 *
 * Build with the flags of camera_model.c: -O3 -ffp-contract=off -fno-fast-math (no -march: no FMA).
 */
#include "camera_model.c"

enum { CAMG_WORDS = 128 };

/* The statistic: stats[(i * 8 + j) * 2] = N_ij, stats[(i * 8 + j) * 2 + 1] = S_ij; all 128 words are written.  out: lens, size
 * and channels; its data is not looked at.  Returns 0, or -1 for an unknown lens / model or a count or range out of bounds. */
int camg_overlap(const cam_camera *cams, int n_in, const float *rotations, const cvm_image *out, float lo, float hi, uint64_t *stats) {
  if (n_in < 1 || n_in > CAM_MAX_SOURCES || out->channels < 1 || out->channels > CAM_MAX_CHANNELS || out->lens.type < 0 || out->lens.type > 4 ||
      !(0.0f <= lo && lo <= hi && hi <= 32768.0f))
    return -1;
  cvm_image img[CAM_MAX_SOURCES] = {0};
  for (int i = 0; i < n_in; ++i) {
    if (cams[i].model != CAM_BROWN && cams[i].model != CAM_FISHEYE) return -1;
    img[i].width = cams[i].width, img[i].height = cams[i].height, img[i].channels = out->channels, img[i].data = cams[i].data;
  }
  for (int w = 0; w < CAMG_WORDS; ++w) stats[w] = 0;
  const int C = out->channels;
  float s[CAM_MAX_CHANNELS];
  for (int y = 0; y < out->height; ++y) {
    for (int x = 0; x < out->width; ++x) {
      float cx = (x + 0.5f) - out->width * 0.5f;
      float cy = (y + 0.5f) - out->height * 0.5f;
      float scx = cx + (0 + 1.0f) / (1 + 1.0f) - 0.5f; /* the one sub-sample of num_samples == 1 */
      float scy = cy + (0 + 1.0f) / (1 + 1.0f) - 0.5f;
      float r[3];
      target_ray(&out->lens, (float)out->width, (float)out->height, scx, scy, r);
      int valid[CAM_MAX_SOURCES];
      uint32_t q[CAM_MAX_SOURCES];
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
        valid[i] = 0, q[i] = 0;
        if (!cam_covered(S, imaged, sx, sy)) continue;
        tap_bilinear(img + i, 0, sx, sy, s);
        float Y = s[0];
        if (C >= 3) Y = (0.25f * s[0] + 0.5f * s[1]) + 0.25f * s[2];
        if (Y >= lo && Y <= hi) {
          valid[i] = 1;
          q[i] = (uint32_t)(Y * 65536.0f);
        }
      }
      for (int i = 0; i < n_in; ++i)
        for (int j = 0; j < n_in; ++j)
          if (valid[i] && valid[j]) {
            stats[(i * 8 + j) * 2] += 1;
            stats[(i * 8 + j) * 2 + 1] += q[i];
          }
    }
  }
  return 0;
}

/* cam_compose with one insertion: right after sampling, s[c] = gains[i] * s[c] for c < min(C, 3). */
int camg_compose(const cam_camera *cams, int n_in, const float *rotations, const float *gains, cvm_image *out, int num_samples,
                 int interpolation, int mode, const float *post, uint8_t *count, uint8_t *coverage) {
  if (n_in < 1 || n_in > CAM_MAX_SOURCES || num_samples < 1 || num_samples > 15 || interpolation < 0 || interpolation > 2 || mode < 0 ||
      mode > 2 || out->channels < 1 || out->channels > CAM_MAX_CHANNELS || out->lens.type < 0 || out->lens.type > 4)
    return -1;
  cvm_image img[CAM_MAX_SOURCES] = {0};
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
            for (int c = 0; c < (C < 3 ? C : 3); ++c) s[c] = gains[i] * s[c]; /* the gain: colour only */
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
          for (int c = 0; c < (C < 3 ? C : 3); ++c) {
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
