// lrp_camera_packed_kernel.h — the packed camera compose kernel (include/lrp.h "calibrated cameras, packed pixels", DESIGN.md
// section 21): several calibrated cameras' frames of 8-bit or binary16 samples composed, with n x n sub-samples per pixel and one
// gain per camera, into one output of 8-bit, binary16 or float samples by one launch.  Included by one unit per
// interpolation (lrp_camera_packed.hip; lrp_camera_packed_unit.hip, units.list) and, for the bicubic sampler, one per source
// format, so that the instantiation sets compile in parallel.
//
// The bytes are those of lrp_decode_pixels_device per camera -> lrp_compose_cameras_gain_device -> lrp_encode_pixels_device with
// float32 staging images of C channels in between.  It is compose_ss_pixel's body (lrp_compose_pixel.h) as camgain_kernel
// instantiates it, between packed_kernel's two ends (lrp_packed_kernel.h).  The body — the sub-sample loops, the camera loop,
// FIRST / MEAN / FEATHER, the divides, the tonemap — is written out here once more, as compose_packed_kernel writes out
// compose_kernel's, and an edit to it there belongs here too: with a tap loader and a store as two more policies of the shared
// function, the kernels that exist would have to be shown not to move, and section 20 records that they do.  The leaves are
// restated nowhere: camera_project and the box test are CameraSources::map, the target is IdealTarget<OutLens>, the samplers are
// sample<> of lrp_device.h with the decoding tap loader PackedTaps, the store is store_packed.
//
// Mapping (gfx950): the 32 x 8 tile, one pixel per lane, tiles in xcd_tile() order; the three loops are wave-uniform and rolled;
// a camera's descriptor and its gain are scalar loads from the kernarg block; a camera no lane's sub-sample needs is skipped by a
// wave-wide test, FIRST leaves the camera loop once every lane has a value.  The two 8-bit tables sit in LDS (1 KiB each),
// loaded by the 256 threads BEFORE any of them leaves; there is no barrier after that — lanes leave the loops at different
// times.  Output lens, sampler, source format and channel lanes (4 for C <= 4, else 8) are template arguments; the camera model,
// the output format, the store width and — per camera — the tap width are wave-uniform run-time switches.
#pragma once

#include "lrp_camera_kernel.h"
#include "lrp_camera_packed.h"
#include "lrp_packed_kernel.h"

namespace lrp {

using CameraPackedKernelFn = void (*)(const CameraPackedParams);

template <int OutLens, int Interp, int CH, int Fmt>
__global__ __launch_bounds__(kComposeThreads) void compose_cam_packed_kernel(const CameraPackedParams P) {
  constexpr int L = texel_lanes<CH>();
  static_assert(kComposeThreads == 256 && kComposeThreads == kPackedThreads, "one thread per entry of an 8-bit table");
  // The tables first: every thread of the workgroup reaches the barrier (the conditions are uniform over the launch).
  __shared__ float lut[256];
  __shared__ float thr[256];
  const bool want_thr = P.out_format == kPackedU8;
  if constexpr (Fmt == kPackedU8) lut[threadIdx.x] = P.decode[threadIdx.x];
  if (want_thr) thr[threadIdx.x] = P.threshold[threadIdx.x];
  if (Fmt == kPackedU8 || want_thr) __syncthreads();

  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;

  const IdealTarget<OutLens> T(P, x, y);
  const int mode = P.mode;
  const int ns = P.num_samples;
  const float ns1 = (float)ns + 1.0f;
  Texel<CH> acc; // the sum of v_j over the covered sub-samples
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  uint32_t m = 0;    // covered sub-samples
  uint32_t seen = 0; // bit i: camera i covers at least one sub-sample

#pragma unroll 1
  for (int ssx = 0; ssx < ns; ++ssx) {
    const float col = T.column(ssx, ns1);
#pragma unroll 1
    for (int ssy = 0; ssy < ns; ++ssy) {
      float rx, ry, rz; // the target ray, once for all cameras
      T.ray(P, col, ssy, ns1, rx, ry, rz);

      // ---- v_j, k_j of this sub-sample
      Texel<CH> v;
#pragma unroll
      for (int c = 0; c < L; ++c) v.v[c] = 0.0f;
      float wsum = 0.0f;
      uint32_t k = 0;
#pragma unroll 1
      for (int i = 0; i < P.n_src; ++i) {
        const CameraSource &S = P.src[i]; // wave-uniform
        const float g = P.gain[i];        // wave-uniform
        float vx = rx, vy = ry, vz = rz;
        if (S.has_rot) {
          vx = S.rot[0] * rx + S.rot[1] * ry + S.rot[2] * rz;
          vy = S.rot[3] * rx + S.rot[4] * ry + S.rot[5] * rz;
          vz = S.rot[6] * rx + S.rot[7] * ry + S.rot[8] * rz;
        }
        const float in_w = (float)S.in_w, in_h = (float)S.in_h;
        float sx, sy;
        const bool covered = CameraSources::map(S, vx, vy, vz, in_w, in_h, sx, sy);
        const bool need = covered && (mode != kComposeFirst || k == 0u);
        if (__builtin_amdgcn_ballot_w64(need) != 0ull) { // a camera no lane's sub-sample needs is not sampled
          if (need) {
            KParams Q; // the sampler's view of camera i: sample<> reads these five fields of a KParams and nothing else
            Q.src = S.data;
            Q.in_w = S.in_w;
            Q.in_h = S.in_h;
            Q.channels = 1; // the samplers' element offsets are texel indices (PackedTaps)
            Q.ch_count = P.channels;
            Texel<CH> s;
            if ((P.in_vec >> i) & 1u) // this camera's taps: one dword / 8-byte load, or one load per sample
              s = sample<Interp, CH, false>(Q, sx, sy, PackedTaps<Fmt, true>{lut, (uint32_t)P.in_pitch, P.in_copy});
            else
              s = sample<Interp, CH, false>(Q, sx, sy, PackedTaps<Fmt, false>{lut, (uint32_t)P.in_pitch, P.in_copy});
#pragma unroll
            for (int c = 0; c < 3; ++c) // the gain: colour only (CameraGainHook, lrp_camgain_kernel.h)
              if (c < P.channels) s.v[c] = g * s.v[c];
            if (mode == kComposeFeather) {
              const float dy = compose_min(sy + 0.5f, (in_h - 0.5f) - sy);
              const float d = compose_min(compose_min(sx + 0.5f, (in_w - 0.5f) - sx), dy);
              const float w = (d < 0x1p-10f) ? 0x1p-10f : d;
#pragma unroll
              for (int c = 0; c < L; ++c) {
                const float t = w * s.v[c];
                v.v[c] = v.v[c] + t;
              }
              wsum = wsum + w;
            } else if (mode == kComposeMean) {
#pragma unroll
              for (int c = 0; c < L; ++c) v.v[c] = v.v[c] + s.v[c];
            } else {
#pragma unroll
              for (int c = 0; c < L; ++c) v.v[c] = s.v[c];
            }
          }
        }
        k += covered ? 1u : 0u;
        seen |= covered ? (1u << i) : 0u;
        // FIRST: every lane has its value (a count plane wants to see all cameras)
        if (mode == kComposeFirst && P.count == nullptr && __builtin_amdgcn_ballot_w64(k == 0u) == 0ull) break;
      }

      if (k != 0u) { // an uncovered sub-sample adds nothing and is not counted
        if (mode != kComposeFirst) {
          const float div = mode == kComposeMean ? (float)k : wsum;
#pragma unroll
          for (int c = 0; c < L; ++c) v.v[c] = v.v[c] / div;
        }
#pragma unroll
        for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] + v.v[c];
        m += 1u;
      }
    }
  }

  if (m == 0u) { // no sub-sample is covered: +0.0f in the C channels before the encode, whatever post is
#pragma unroll
    for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  } else {
    const float r = 1.0f / (float)m;
#pragma unroll
    for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] * r;
    if (P.has_post) { // fused post_process: the first min(C, 3) channels
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c < P.channels) acc.v[c] = tonemap(acc.v[c], P.exposure, P.reinhard);
    }
  }
  const uint32_t px_index = (uint32_t)y * (uint32_t)P.out_w + (uint32_t)x;
  store_packed<CH>(P, thr, px_index, acc);
  if (P.count != nullptr) P.count[px_index] = (uint8_t)__builtin_popcount(seen);
  if (P.coverage != nullptr) P.coverage[px_index] = (uint8_t)m;
}

// The kernels: one per output lens id (0 .. kLensIds - 1; the extension lenses are gated by the caller's validation), per
// interpolation, source format and lane count.
template <int Interp, int CH, int Fmt, int... OutLens>
constexpr std::array<CameraPackedKernelFn, kLensIds> camera_packed_kernel_table(std::integer_sequence<int, OutLens...>) {
  return {{compose_cam_packed_kernel<OutLens, Interp, CH, Fmt>...}};
}
// The kernel of output lens out_lens; nullptr: no such lens.
template <int Interp, int CH, int Fmt> CameraPackedKernelFn camera_packed_kernel(int out_lens) {
  static constexpr std::array<CameraPackedKernelFn, kLensIds> table =
      camera_packed_kernel_table<Interp, CH, Fmt>(std::make_integer_sequence<int, kLensIds>{});
  if (out_lens < 0 || out_lens >= kLensIds) return nullptr;
  return table[out_lens];
}

// One source format's kernels: the unit of the split of the bicubic instantiations (units.list, lrp_camera_packed_bc*.o).
// P: as launch_compose_cameras_packed (lrp_camera_packed.hip) completed it.
template <int Interp, int Fmt> hipError_t launch_camera_packed_fmt(const CameraPackedParams &P, int out_lens, hipStream_t stream) {
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  const CameraPackedKernelFn fn = P.channels <= 4 ? camera_packed_kernel<Interp, 4, Fmt>(out_lens) : camera_packed_kernel<Interp, 0, Fmt>(out_lens);
  if (!fn) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

template <int Interp> hipError_t launch_camera_packed_interp(const CameraPackedParams &P, int in_format, int out_lens, hipStream_t stream) {
  if (in_format == kPackedU8) return launch_camera_packed_fmt<Interp, kPackedU8>(P, out_lens, stream);
  return launch_camera_packed_fmt<Interp, kPackedF16>(P, out_lens, stream);
}

// launch_camera_packed_fmt as a bilinear / bicubic unit of units.list compiles it: defined and instantiated by
// lrp_camera_packed_unit.hip, declared only for the launcher.
template <int Interp, int Fmt> hipError_t launch_camera_packed_unit(const CameraPackedParams &P, int out_lens, hipStream_t stream);
} // namespace lrp
