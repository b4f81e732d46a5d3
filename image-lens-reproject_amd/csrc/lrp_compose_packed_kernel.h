// lrp_compose_packed_kernel.h — the packed compose kernel (include/lrp.h "compose, packed pixels"): several
// sources of 8-bit or binary16 samples composed into one output of 8-bit, binary16 or float samples by one launch.  Included by
// one unit per interpolation (lrp_compose_packed.hip; lrp_compose_packed_unit.hip, units.list) and, for the bicubic sampler,
// one per source format, so that the instantiation sets compile in parallel.
//
// The bytes are those of lrp_decode_pixels_device per source -> lrp_compose_device -> lrp_encode_pixels_device with float32
// staging images of C channels in between.  It is compose_kernel's body (lrp_compose_kernel.h) between packed_kernel's two ends
// (lrp_packed_kernel.h).  The body — source loop, FIRST / MEAN / FEATHER, divide, tonemap — is written out here a second time,
// and an edit to it there belongs here too: folded onto one function, kernels of both moved registers.
// The leaves are restated nowhere: the coverage test and min are compose_covered / compose_min, the lens math is target_ray /
// ray_to_source, the samplers are sample<> of lrp_device.h with the decoding tap loader PackedTaps, the store is store_packed.
//
// Mapping (gfx950): the 32 x 8 tile, one pixel per lane, tiles in xcd_tile() order; the wave-uniform source loop reads its
// descriptor from kernarg with scalar loads, a source no active lane needs is skipped by a wave-wide test, FIRST leaves the
// loop once every active lane has a value.  The two 8-bit tables sit in LDS (1 KiB each), loaded by the 256 threads BEFORE
// any of them leaves; there is no barrier after that — lanes leave the source loop at different times.  Source format, channel
// lanes (4 for C <= 4, else 8) and sampler are template arguments; the output format, the store width and — per source — the
// tap width are wave-uniform run-time switches.
#pragma once

#include "lrp_compose_kernel.h"
#include "lrp_compose_packed.h"
#include "lrp_packed_kernel.h"

namespace lrp {

using ComposePackedKernelFn = void (*)(const ComposePackedParams);

template <int OutLens, int InMode, int Interp, int CH, int Fmt>
__global__ __launch_bounds__(kComposeThreads) void compose_packed_kernel(const ComposePackedParams P) {
  constexpr bool Loop = (InMode == kInEquirectLoop);
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

  // pixel centre and the one sub-sample of a num_samples == 1 call, then the target ray, once for all sources (compose_kernel)
  const float scx = ((((float)x + 0.5f) - (float)P.out_w * 0.5f) + 0.5f) - 0.5f;
  const float scy = ((((float)y + 0.5f) - (float)P.out_h * 0.5f) + 0.5f) - 0.5f;
  float rx, ry, rz;
  target_ray<OutLens>(P.out_lens, (float)P.out_w, (float)P.out_h, scx, scy, rx, ry, rz);

  const int mode = P.mode;
  Texel<CH> acc;
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  float wsum = 0.0f;
  uint32_t k = 0;

#pragma unroll 1
  for (int i = 0; i < P.n_src; ++i) {
    const ComposePackedSource &S = P.src[i]; // wave-uniform
    float vx = rx, vy = ry, vz = rz;
    if (S.has_rot) {
      vx = S.rot[0] * rx + S.rot[1] * ry + S.rot[2] * rz;
      vy = S.rot[3] * rx + S.rot[4] * ry + S.rot[5] * rz;
      vz = S.rot[6] * rx + S.rot[7] * ry + S.rot[8] * rz;
    }
    const float in_w = (float)S.in_w, in_h = (float)S.in_h;
    float px, py;
    ray_to_source<InMode>(S.lens, in_w, in_h, vx, vy, vz, px, py);
    const float sx = (px - 0.5f) + in_w * 0.5f;
    const float sy = (py - 0.5f) + in_h * 0.5f;
    const bool covered = compose_covered<InMode>(sx, sy, vz, in_w, in_h);
    const bool need = covered && (mode != kComposeFirst || k == 0u);
    if (__builtin_amdgcn_ballot_w64(need) != 0ull) { // a source no lane of the wavefront needs is not sampled
      if (need) {
        KParams Q; // the sampler's view of source i: sample<> reads these five fields of a KParams and nothing else
        Q.src = static_cast<const float *>(S.data);
        Q.in_w = S.in_w;
        Q.in_h = S.in_h;
        Q.channels = 1; // the samplers' element offsets are texel indices (PackedTaps)
        Q.ch_count = P.channels;
        Texel<CH> s;
        if (S.in_vec) // this source's taps: one dword / 8-byte load, or one load per sample
          s = sample<Interp, CH, Loop>(Q, sx, sy, PackedTaps<Fmt, true>{lut, (uint32_t)P.in_pitch, P.in_copy});
        else
          s = sample<Interp, CH, Loop>(Q, sx, sy, PackedTaps<Fmt, false>{lut, (uint32_t)P.in_pitch, P.in_copy});
        if (mode == kComposeFeather) {
          const float dy = compose_min(sy + 0.5f, (in_h - 0.5f) - sy);
          float m = dy;
          if constexpr (!Loop) m = compose_min(compose_min(sx + 0.5f, (in_w - 0.5f) - sx), dy);
          const float w = (m < 0x1p-10f) ? 0x1p-10f : m;
#pragma unroll
          for (int c = 0; c < L; ++c) {
            const float t = w * s.v[c];
            acc.v[c] = acc.v[c] + t;
          }
          wsum = wsum + w;
        } else if (mode == kComposeMean) {
#pragma unroll
          for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] + s.v[c];
        } else {
#pragma unroll
          for (int c = 0; c < L; ++c) acc.v[c] = s.v[c];
        }
      }
    }
    k += covered ? 1u : 0u;
    // FIRST: every lane has its value (a count plane wants k of all sources)
    if (mode == kComposeFirst && P.count == nullptr && __builtin_amdgcn_ballot_w64(k == 0u) == 0ull) break;
  }

  if (k == 0u) { // no source covers the pixel: +0.0f in the C channels before the encode, whatever post is
#pragma unroll
    for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  } else {
    if (mode != kComposeFirst) {
      const float div = mode == kComposeMean ? (float)k : wsum;
#pragma unroll
      for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] / div;
    }
    if (P.has_post) { // fused post_process: the first min(C, 3) channels
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c < P.channels) acc.v[c] = tonemap(acc.v[c], P.exposure, P.reinhard);
    }
  }
  const uint32_t px_index = (uint32_t)y * (uint32_t)P.out_w + (uint32_t)x;
  store_packed<CH>(P, thr, px_index, acc);
  if (P.count != nullptr) P.count[px_index] = (uint8_t)k;
}

// The cells: all 30 (the extension lenses are gated by the caller's validation), per interpolation, source format and lane
// count, in the layout of the compose kernel's table — entry out_lens * kInModes + in_mode.
template <int Interp, int CH, int Fmt, int Cell> constexpr ComposePackedKernelFn compose_packed_cell_entry() {
  if constexpr (is_lens_id(Cell / kInModes))
    return compose_packed_kernel<Cell / kInModes, Cell % kInModes, Interp, CH, Fmt>;
  else
    return nullptr;
}
template <int Interp, int CH, int Fmt, int... Cell>
constexpr std::array<ComposePackedKernelFn, kLensIds * kInModes> compose_packed_cell_table(std::integer_sequence<int, Cell...>) {
  return {{compose_packed_cell_entry<Interp, CH, Fmt, Cell>()...}};
}
template <int Interp, int CH, int Fmt> ComposePackedKernelFn compose_packed_cell_kernel(int out_lens, int in_mode) {
  static constexpr std::array<ComposePackedKernelFn, kLensIds * kInModes> table =
      compose_packed_cell_table<Interp, CH, Fmt>(std::make_integer_sequence<int, kLensIds * kInModes>{});
  if (out_lens < 0 || out_lens >= kLensIds || in_mode < 0 || in_mode >= kInModes) return nullptr;
  return table[out_lens * kInModes + in_mode];
}

// One source format's kernels: the unit of the split of the bicubic instantiations (units.list, lrp_compose_packed_bc*.o).
template <int Interp, int Fmt> hipError_t launch_compose_packed_fmt(const ComposePackedParams &P, int out_lens, int in_mode, hipStream_t stream) {
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  const ComposePackedKernelFn fn =
      P.channels <= 4 ? compose_packed_cell_kernel<Interp, 4, Fmt>(out_lens, in_mode) : compose_packed_cell_kernel<Interp, 0, Fmt>(out_lens, in_mode);
  if (!fn) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x)), block(kComposeThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

// P: as launch_compose_packed (lrp_compose_packed.hip) completed it.
template <int Interp> hipError_t launch_compose_packed_interp(const ComposePackedParams &P, int in_format, int out_lens, int in_mode, hipStream_t stream) {
  if (in_format == kPackedU8) return launch_compose_packed_fmt<Interp, kPackedU8>(P, out_lens, in_mode, stream);
  return launch_compose_packed_fmt<Interp, kPackedF16>(P, out_lens, in_mode, stream);
}

// launch_compose_packed_fmt as a bilinear / bicubic unit of units.list compiles it: defined and instantiated by
// lrp_compose_packed_unit.hip, declared only for the launcher.
template <int Interp, int Fmt> hipError_t launch_compose_packed_unit(const ComposePackedParams &P, int out_lens, int in_mode, hipStream_t stream);
} // namespace lrp
