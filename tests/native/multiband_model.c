/*
 * multiband_model.c — CPU model of multi-band blending across a camera rig (include/lrp.h "multi-band blending across a camera
 * rig"), written out per pixel from the header's definition: the labels, then per camera its level-0
 * layer, the reduce / expand pyramid, the accumulation in ascending camera order, and the collapse.  The level-0 layers are
 * cam_compose / camg_compose of tests/native/camera_model.c and camera_gain_model.c, included textually and unedited.  Test
 * infrastructure.
 *
 * Build with the flags of camera_model.c: -O3 -ffp-contract=off -fno-fast-math (no -march: no FMA).
 */
#include <stdlib.h>

#include "camera_gain_model.c"

enum { MBM_MAX_BANDS = 8, MBM_MAX_CHANNELS = 4, MBM_NO_CAMERA = 255 };

static int mbm_x(int j, int w, int wrap) {
  if (wrap) {
    int r = j % w;
    return r < 0 ? r + w : r;
  }
  return j < 0 ? 0 : (j >= w ? w - 1 : j);
}
static int mbm_y(int j, int h) { return j < 0 ? 0 : (j >= h ? h - 1 : j); }

static float mbm_tap5(float pm2, float pm1, float p0, float p1, float p2) { return (((pm2 + p2) + 4.0f * (pm1 + p1)) + 6.0f * p0) * 0.0625f; }

/* src: w x h x P interleaved -> dst: cw x ch x P */
static void mbm_reduce(const float *src, int w, int h, int P, int wrap, float *dst, int cw, int ch) {
  float *hor = (float *)malloc(sizeof(float) * (size_t)cw * h * P);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < cw; ++x)
      for (int c = 0; c < P; ++c) {
        const float *row = src + (size_t)y * w * P + c;
        hor[((size_t)y * cw + x) * P + c] = mbm_tap5(row[(size_t)mbm_x(2 * x - 2, w, wrap) * P], row[(size_t)mbm_x(2 * x - 1, w, wrap) * P],
                                                     row[(size_t)mbm_x(2 * x, w, wrap) * P], row[(size_t)mbm_x(2 * x + 1, w, wrap) * P],
                                                     row[(size_t)mbm_x(2 * x + 2, w, wrap) * P]);
      }
  for (int y = 0; y < ch; ++y)
    for (int x = 0; x < cw; ++x)
      for (int c = 0; c < P; ++c) {
        const float *col = hor + (size_t)x * P + c;
        const size_t pitch = (size_t)cw * P;
        dst[((size_t)y * cw + x) * P + c] = mbm_tap5(col[mbm_y(2 * y - 2, h) * pitch], col[mbm_y(2 * y - 1, h) * pitch], col[mbm_y(2 * y, h) * pitch],
                                                     col[mbm_y(2 * y + 1, h) * pitch], col[mbm_y(2 * y + 2, h) * pitch]);
      }
  free(hor);
}

/* src: cw x ch x P -> dst: w x h x P */
static void mbm_expand(const float *src, int cw, int ch, int P, int wrap, float *dst, int w, int h) {
  float *hor = (float *)malloc(sizeof(float) * (size_t)w * ch * P);
  for (int y = 0; y < ch; ++y)
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < P; ++c) {
        const float *row = src + (size_t)y * cw * P + c;
        const int i = x >> 1;
        const float c0 = row[(size_t)mbm_x(i, cw, wrap) * P], c1 = row[(size_t)mbm_x(i + 1, cw, wrap) * P];
        float e;
        if (x & 1) {
          e = (c0 + c1) * 0.5f;
        } else {
          const float cm = row[(size_t)mbm_x(i - 1, cw, wrap) * P];
          e = ((cm + c1) + 6.0f * c0) * 0.125f;
        }
        hor[((size_t)y * w + x) * P + c] = e;
      }
  const size_t pitch = (size_t)w * P;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < P; ++c) {
        const float *col = hor + (size_t)x * P + c;
        const int i = y >> 1;
        const float c0 = col[mbm_y(i, ch) * pitch], c1 = col[mbm_y(i + 1, ch) * pitch];
        float e;
        if (y & 1) {
          e = (c0 + c1) * 0.5f;
        } else {
          const float cm = col[mbm_y(i - 1, ch) * pitch];
          e = ((cm + c1) + 6.0f * c0) * 0.125f;
        }
        dst[((size_t)y * w + x) * P + c] = e;
      }
  free(hor);
}

/* The labels and the count plane alone.  Returns 0 or -1. */
int mbm_labels(const cam_camera *cams, int n_in, const float *rotations, const cvm_image *out, uint8_t *count, uint8_t *label) {
  if (n_in < 1 || n_in > CAM_MAX_SOURCES || out->lens.type < 0 || out->lens.type > 4) return -1;
  for (int i = 0; i < n_in; ++i)
    if (cams[i].model != CAM_BROWN && cams[i].model != CAM_FISHEYE) return -1;
  for (int y = 0; y < out->height; ++y) {
    for (int x = 0; x < out->width; ++x) {
      float cx = (x + 0.5f) - out->width * 0.5f;
      float cy = (y + 0.5f) - out->height * 0.5f;
      float scx = cx + (0 + 1.0f) / (1 + 1.0f) - 0.5f; /* the one sub-sample of num_samples == 1 */
      float scy = cy + (0 + 1.0f) / (1 + 1.0f) - 0.5f;
      float r[3];
      target_ray(&out->lens, (float)out->width, (float)out->height, scx, scy, r);
      int k = 0, winner = MBM_NO_CAMERA;
      float best = 0.0f;
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
        float dy = cam_min(sy + 0.5f, ((float)S->height - 0.5f) - sy);
        float d = cam_min(cam_min(sx + 0.5f, ((float)S->width - 0.5f) - sx), dy);
        float w = (d < 0x1p-10f) ? 0x1p-10f : d;
        if (k == 0 || w > best) best = w, winner = i;
        ++k;
      }
      ptrdiff_t at = (ptrdiff_t)y * out->width + x;
      count[at] = (uint8_t)k;
      label[at] = (uint8_t)winner;
    }
  }
  return 0;
}

/* gains: n_in floats or NULL; post: {exposure, reinhard} or NULL; count, label: out->width * out->height bytes each, required.
 * Returns 0, or -1 for an argument out of range. */
int mbm_compose(const cam_camera *cams, int n_in, const float *rotations, const float *gains, cvm_image *out, int interpolation, int num_bands,
                const float *post, uint8_t *count, uint8_t *label) {
  const int W = out->width, H = out->height, C = out->channels, B = num_bands;
  if (C < 1 || C > MBM_MAX_CHANNELS || B < 0 || B > MBM_MAX_BANDS || interpolation < 0 || interpolation > 2) return -1;
  if (mbm_labels(cams, n_in, rotations, out, count, label) != 0) return -1;
  const int wrap = source_wraps(&out->lens);
  int w[MBM_MAX_BANDS + 1], h[MBM_MAX_BANDS + 1];
  float *G[MBM_MAX_BANDS + 1], *M[MBM_MAX_BANDS + 1], *A[MBM_MAX_BANDS + 1], *S[MBM_MAX_BANDS + 1];
  w[0] = W, h[0] = H;
  for (int k = 1; k <= B; ++k) w[k] = (w[k - 1] + 1) >> 1, h[k] = (h[k - 1] + 1) >> 1;
  for (int k = 0; k <= B; ++k) {
    size_t px = (size_t)w[k] * h[k];
    G[k] = (float *)malloc(sizeof(float) * px * C), M[k] = (float *)malloc(sizeof(float) * px);
    A[k] = (float *)malloc(sizeof(float) * px * C), S[k] = (float *)malloc(sizeof(float) * px);
    for (size_t j = 0; j < px * C; ++j) A[k][j] = 0.0f;
    for (size_t j = 0; j < px; ++j) S[k][j] = 0.0f;
  }
  float *E = (float *)malloc(sizeof(float) * (size_t)W * H * C);
  int rc = 0;
  for (int i = 0; i < n_in && rc == 0; ++i) {
    cvm_image layer = *out;
    layer.data = G[0];
    const float *rm = rotations ? rotations + 9 * i : NULL;
    rc = gains ? camg_compose(cams + i, 1, rm, gains + i, &layer, 1, interpolation, CAM_FIRST, NULL, NULL, NULL)
               : cam_compose(cams + i, 1, rm, &layer, 1, interpolation, CAM_FIRST, NULL, NULL, NULL);
    if (rc != 0) break;
    for (size_t j = 0; j < (size_t)W * H; ++j) M[0][j] = (label[j] == i) ? 1.0f : 0.0f;
    for (int k = 0; k < B; ++k) {
      mbm_reduce(G[k], w[k], h[k], C, wrap, G[k + 1], w[k + 1], h[k + 1]);
      mbm_reduce(M[k], w[k], h[k], 1, wrap, M[k + 1], w[k + 1], h[k + 1]);
    }
    for (int k = 0; k <= B; ++k) {
      if (k < B) mbm_expand(G[k + 1], w[k + 1], h[k + 1], C, wrap, E, w[k], h[k]);
      for (size_t j = 0; j < (size_t)w[k] * h[k]; ++j) {
        for (int c = 0; c < C; ++c) {
          float l = (k < B) ? G[k][j * C + c] - E[j * C + c] : G[k][j * C + c];
          float t = (M[k][j] == 0.0f) ? 0.0f : M[k][j] * l;
          A[k][j * C + c] = A[k][j * C + c] + t;
        }
        S[k][j] = S[k][j] + M[k][j];
      }
    }
  }
  if (rc == 0) {
    for (int k = B; k >= 0; --k) { /* R_k over A_k */
      if (k < B) mbm_expand(A[k + 1], w[k + 1], h[k + 1], C, wrap, E, w[k], h[k]);
      for (size_t j = 0; j < (size_t)w[k] * h[k]; ++j)
        for (int c = 0; c < C; ++c) {
          float n = (S[k][j] > 0.0f) ? A[k][j * C + c] / S[k][j] : 0.0f;
          A[k][j * C + c] = (k < B) ? n + E[j * C + c] : n;
        }
    }
    for (size_t j = 0; j < (size_t)W * H; ++j) {
      float *dst = out->data + j * C;
      if (label[j] == MBM_NO_CAMERA) {
        for (int c = 0; c < C; ++c) dst[c] = 0.0f;
        continue;
      }
      for (int c = 0; c < C; ++c) dst[c] = A[0][j * C + c];
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
  }
  free(E);
  for (int k = 0; k <= B; ++k) free(G[k]), free(M[k]), free(A[k]), free(S[k]);
  return rc;
}
