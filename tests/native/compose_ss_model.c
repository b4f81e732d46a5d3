/*
 * compose_ss_model.c — CPU model of supersampled compose (include/lrp.h "compose, supersampled"): the
 * definition written out per pixel.  The lens functions, samplers and coverage test are those of tests/native/coverage_model.c,
 * included textually and unedited: the GPU coverage tests pin that model's per-sub-sample coordinates to the kernels', and
 * tests/test_coverage.py its render to the oracle.  Test infrastructure.
 *
 * Build with the flags of coverage_model.c: -O3 -ffp-contract=off -fno-fast-math (no -march: no FMA).
 */
#include "coverage_model.c"

enum { CSM_FIRST = 0, CSM_MEAN = 1, CSM_FEATHER = 2, CSM_MAX_SOURCES = 8, CSM_MAX_CHANNELS = 64 };

/* min(a, b) of include/lrp.h "compose" */
static float csm_min(float a, float b) { return (b < a) ? b : a; }

/* ins: n_in images; rotations: n_in x 9 or NULL; post: {exposure, reinhard} or NULL; count / coverage: out->width * out->height
 * bytes or NULL.  Returns 0, or -1 for an unknown lens / sampler / mode or a count out of range. */
int csm_compose(const cvm_image *ins, int n_in, const float *rotations, cvm_image *out, int num_samples, int interpolation, int mode,
                const float *post, uint8_t *count, uint8_t *coverage) {
  if (n_in < 1 || n_in > CSM_MAX_SOURCES || num_samples < 1 || num_samples > 15 || interpolation < 0 || interpolation > 2 || mode < 0 ||
      mode > 2 || out->channels < 1 || out->channels > CSM_MAX_CHANNELS || out->lens.type < 0 || out->lens.type > 4)
    return -1;
  int loop[CSM_MAX_SOURCES];
  for (int i = 0; i < n_in; ++i) {
    if (ins[i].lens.type < 0 || ins[i].lens.type > 4 || ins[i].channels != out->channels) return -1;
    loop[i] = source_wraps(&ins[i].lens);
  }
  const int n = num_samples, C = out->channels;
  float acc[CSM_MAX_CHANNELS], v[CSM_MAX_CHANNELS], s[CSM_MAX_CHANNELS];
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
          /* v_j, k_j: the compose definition for this sub-sample */
          int k = 0;
          float wsum = 0.0f;
          for (int c = 0; c < C; ++c) v[c] = 0.0f;
          for (int i = 0; i < n_in; ++i) {
            const cvm_image *in = ins + i;
            float sx, sy, vz;
            cvm_source_ray(in, out, rotations ? rotations + 9 * i : NULL, scx, scy, &sx, &sy, &vz);
            if (!covered(in, loop[i], sx, sy, vz)) continue;
            seen |= 1u << i;
            ++k;
            if (mode == CSM_FIRST && k > 1) continue;
            if (interpolation == 0)
              tap_nearest(in, loop[i], sx, sy, s);
            else if (interpolation == 1)
              tap_bilinear(in, loop[i], sx, sy, s);
            else
              tap_bicubic(in, loop[i], sx, sy, s);
            if (mode == CSM_FIRST) {
              for (int c = 0; c < C; ++c) v[c] = s[c];
            } else if (mode == CSM_MEAN) {
              for (int c = 0; c < C; ++c) v[c] = v[c] + s[c];
            } else {
              float dy = csm_min(sy + 0.5f, ((float)in->height - 0.5f) - sy);
              float d = loop[i] ? dy : csm_min(csm_min(sx + 0.5f, ((float)in->width - 0.5f) - sx), dy);
              float w = (d < 0x1p-10f) ? 0x1p-10f : d;
              for (int c = 0; c < C; ++c) {
                float t = w * s[c];
                v[c] = v[c] + t;
              }
              wsum = wsum + w;
            }
          }
          if (k == 0) continue;
          if (mode != CSM_FIRST) {
            float div = mode == CSM_MEAN ? (float)k : wsum;
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
        float r = 1.0f / (float)m;
        for (int c = 0; c < C; ++c) dst[c] = acc[c] * r;
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
