// lrp_multiband.h — argument blocks, tile shapes and the scratch layout of multi-band blending (include/lrp.h "multi-band
// blending across a camera rig"), shared by lrp_capi.cpp and the lrp_multiband*.hip units.  Plain PODs
// passed by value in kernarg: wave-uniform, read with scalar loads.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "lrp_camera.h"

namespace lrp {

constexpr int kMultibandMaxBands = 8;     // LRP_MULTIBAND_MAX_BANDS
constexpr int kMultibandMaxChannels = 4;  // colour channels of one call
constexpr int kMultibandNoCamera = 255;   // LRP_MULTIBAND_NO_CAMERA
constexpr int kMultibandMaxHeight = 8 * 65535; // rows of 8-row tiles a 2-D launch grid can hold

// Tiles: every pyramid kernel is 256 threads on a 32 x 8 tile of the level it WRITES, one texel per lane.
constexpr int kMbTileW = 32;
constexpr int kMbTileH = 8;
constexpr int kMbThreads = kMbTileW * kMbTileH;
// reduce: the fine-level window of a 32 x 8 coarse tile with its 2-texel halo, 67 x 19, in an LDS row of 68 floats whose even
// columns come first (kMbReduceHalf of them) and whose odd columns follow, so that the taps 2x - 2, 2x, 2x + 2 of neighbouring
// lanes are neighbouring words; then the horizontal pass, 32 x 19.  Per plane; a launch holds C + 1 planes.
constexpr int kMbReduceCols = 2 * kMbTileW + 3; // 67
constexpr int kMbReduceRows = 2 * kMbTileH + 3; // 19
constexpr int kMbReduceHalf = 34;
constexpr int kMbReducePitch = 2 * kMbReduceHalf; // 68
constexpr int kMbReducePlaneFloats = kMbReduceRows * (kMbReducePitch + kMbTileW); // 1900
constexpr int mb_reduce_lds_bytes(int channels) { return (channels + 1) * kMbReducePlaneFloats * 4; }
// expand (Laplacian-accumulate, collapse): the coarse-level window of a 32 x 8 fine tile with its 1-texel halo, 18 x 6, then
// the horizontal pass, 32 x 6.  Per colour channel.
constexpr int kMbExpandCols = kMbTileW / 2 + 2; // 18
constexpr int kMbExpandRows = kMbTileH / 2 + 2; // 6
constexpr int kMbExpandPlaneFloats = kMbExpandRows * (kMbExpandCols + kMbTileW); // 300
constexpr int mb_expand_lds_bytes(int channels) { return channels * kMbExpandPlaneFloats * 4; }

// The label kernel: compose_cam_kernel's geometry at num_samples == 1, no sampling (src[i].data is not looked at).
struct MultibandLabelParams {
  uint8_t *label; // the winner per pixel, kMultibandNoCamera where no camera covers it
  uint8_t *count; // the number of covering cameras
  int32_t out_w, out_h;
  int32_t n_src;
  int32_t tiles_x, tiles_y; // (launch_compose_tiles' fields)
  LensP out_lens;
  CameraSource src[kComposeMaxSources];
};

// reduce: level k (w x h) -> level k + 1 (cw x ch), C colour channels and the weight plane.
struct MultibandReduceParams {
  const float *g;       // G_k, w x h x C interleaved
  const float *m;       // M_k, w x h; null at level 0, where M_0 = (label == cam)
  const uint8_t *label; // level 0 only
  float *cg;            // G_{k+1}
  float *cm;            // M_{k+1}
  int32_t w, h, cw, ch;
  int32_t cam;
  int32_t wrap; // X_k is j modulo w (a full-turn equirectangular target), else a clamp
};

// Laplacian-accumulate: A_k += M_k * (G_k - E(G_{k+1})) (+0.0f where M_k == 0), S_k += M_k; `top`: L_B = G_B; `first`: A_k and S_k start at +0.0f.
struct MultibandLapParams {
  const float *g;       // G_k
  const float *m;       // M_k, null at level 0
  const uint8_t *label; // level 0 only
  const float *cg;      // G_{k+1}, cw x ch; not read when top
  float *a;             // A_k, w x h x C
  float *s;             // S_k, w x h
  int32_t w, h, cw, ch;
  int32_t cam;
  int32_t wrap;
  int32_t top, first;
};

// collapse: R_k = N_k + E(R_{k+1}), written over A_k, or, at level 0, into the output with the label rule and post.
struct MultibandCollapseParams {
  const float *a;       // A_k
  const float *s;       // S_k
  const float *cr;      // R_{k+1}, cw x ch; not read when top
  float *dst;           // R_k: A_k itself, or the output at level 0
  const uint8_t *label; // level 0: kMultibandNoCamera pixels are +0.0f; null at the other levels
  int32_t w, h, cw, ch;
  int32_t wrap;
  int32_t top;
  int32_t has_post;
  float exposure, reinhard;
};

// The scratch buffer of one call, every region at a multiple of 256 bytes: per level k = 0 .. B one camera's G_k (C floats per
// texel) and, for k > 0, M_k; the accumulators A_k (C floats per texel; R_k is written over it) and S_k; then the label and the
// count plane, used where the caller passes none.
struct MultibandLayout {
  int32_t w[kMultibandMaxBands + 1], h[kMultibandMaxBands + 1];
  size_t g[kMultibandMaxBands + 1], m[kMultibandMaxBands + 1], a[kMultibandMaxBands + 1], s[kMultibandMaxBands + 1];
  size_t label, count, total;
};

inline size_t mb_round256(size_t n) { return (n + 255) & ~(size_t)255; }

inline MultibandLayout multiband_layout(int width, int height, int channels, int num_bands) {
  MultibandLayout L = {};
  size_t at = 0;
  int w = width, h = height;
  for (int k = 0; k <= num_bands; ++k) {
    L.w[k] = w, L.h[k] = h;
    const size_t px = (size_t)w * (size_t)h;
    L.g[k] = at, at += mb_round256(px * (size_t)channels * 4);
    L.m[k] = at, at += k > 0 ? mb_round256(px * 4) : 0;
    L.a[k] = at, at += mb_round256(px * (size_t)channels * 4);
    L.s[k] = at, at += mb_round256(px * 4);
    w = (w + 1) >> 1, h = (h + 1) >> 1;
  }
  const size_t px0 = (size_t)width * (size_t)height;
  L.label = at, at += mb_round256(px0);
  L.count = at, at += mb_round256(px0);
  L.total = at;
  return L;
}

} // namespace lrp
