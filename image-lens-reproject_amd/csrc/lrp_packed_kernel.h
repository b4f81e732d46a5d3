// lrp_packed_kernel.h — the packed-pixel kernel (include/lrp.h "packed pixels"): a source of 8-bit or
// binary16 samples reprojected into an output of 8-bit, binary16 or float samples by one launch.  Included by one unit
// per interpolation (lrp_packed.hip; lrp_packed_unit.hip twice, units.list) so that the three instantiation sets compile in
// parallel.
//
// The bytes are those of lrp_decode_pixels_device -> lrp_reproject_device -> lrp_encode_pixels_device with float32 staging
// images of C channels in between.  Nothing is restated: the lens math is source_position, the samplers are sample<> of
// lrp_device.h with a tap loader that decodes (PackedTaps below, in place of FloatTaps), the 8-bit tables and the threshold
// search are the conversion kernels' (lrp_pixel_codec.h), the half conversion is include/lrp_half.h.
//
// Mapping (gfx950): the 32 x 8 tile of lrp_kernel_impl.h, one pixel per lane, tiles in xcd_tile() order, that kernel's
// num_samples loop.  The two 8-bit tables sit in LDS (1 KiB each, loaded by the 256 threads before any of them leaves).
// Source format, channel lanes (4 for C <= 4, else 8) and sampler are template arguments; the output format, the tap and
// store widths and the geometry-cache write are wave-uniform run-time switches.
#pragma once

#include "../../include/lrp_half.h"
#include "lrp_cells.h"
#include "lrp_device.h"
#include "lrp_packed.h"
#include "lrp_pixel_codec.h"

namespace lrp {

constexpr int kPackedTileW = 32;
constexpr int kPackedTileH = 8;
constexpr int kPackedThreads = kPackedTileW * kPackedTileH; // 256 = 4 wavefronts = the entries of an 8-bit table

using PackedKernelFn = void (*)(const PackedParams);
static_assert(kPackedMaxChannels == kMaxDynChannels, "lrp_packed.h states the limit of lrp_device.h");

// The tap loader of a packed source.  The samplers hand it the texel's element offset for a source of ONE channel
// (KParams::channels == 1), i.e. the texel index; the first `copy` samples are decoded, the other lanes are +0.0f taps (what
// decode_kernel stages for them) that go through the sampler's arithmetic.  Vec: four samples per texel at an aligned base —
// one dword (8-bit) / one 8-byte load (half) per tap; else one byte / short load per sample.
template <int Fmt, bool Vec> struct PackedTaps {
  const float *lut; // LDS: the 8-bit decode table (Fmt == kPackedU8)
  uint32_t pitch;   // bytes per texel
  int copy;
  static __device__ __forceinline__ float half_value(uint32_t h) { return __uint_as_float(lrp_half_to_float_bits((uint16_t)h)); }
  template <int CH> __device__ __forceinline__ Texel<CH> load(const float *__restrict__ src, uint32_t texel, int) const {
    constexpr int L = texel_lanes<CH>();
    Texel<CH> t;
#pragma unroll
    for (int c = 0; c < L; ++c) t.v[c] = 0.0f;
    const uint8_t *const p = reinterpret_cast<const uint8_t *>(src) + texel * pitch;
    if constexpr (Vec && Fmt == kPackedU8) {
      const uint32_t q = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < copy) t.v[c] = lut[(q >> (8 * c)) & 0xffu];
    } else if constexpr (Vec) {
      const uint2 q = *reinterpret_cast<const uint2 *>(p);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t w = c < 2 ? q.x : q.y;
        if (c < copy) t.v[c] = half_value((c & 1) ? (w >> 16) : (w & 0xffffu));
      }
    } else {
#pragma unroll
      for (int c = 0; c < L; ++c)
        if (c < copy) {
          if constexpr (Fmt == kPackedU8)
            t.v[c] = lut[p[c]];
          else
            t.v[c] = half_value(reinterpret_cast<const uint16_t *>(p)[c]);
        }
    }
    return t;
  }
};

// One output pixel in out_format: the first out_copy samples encoded as encode_kernel does, out_fill behind them.  Four
// samples at an aligned base leave as one store; anything else as one store per sample.  Non-temporal, like store_texel.
// Out: the kernarg block of the calling kernel — PackedParams, or ComposePackedParams (lrp_compose_packed.h) — of which the
// output fields dst, out_pitch, out_copy, out_channels, out_format, out_fill and out_vec are read.
template <int CH, class Out> __device__ __forceinline__ void store_packed(const Out &P, const float *thr, uint32_t px, const Texel<CH> &t) {
  constexpr int L = texel_lanes<CH>();
  uint8_t *const o = static_cast<uint8_t *>(P.dst) + px * (uint32_t)P.out_pitch;
  const int copy = P.out_copy, n = P.out_channels;
  if (P.out_format == kPackedU8) {
    uint32_t code[L];
#pragma unroll
    for (int c = 0; c < L; ++c) code[c] = c < copy ? (uint32_t)u8_gamma_code(thr, t.v[c]) : (P.out_fill & 0xffu);
    if (P.out_vec) {
      __builtin_nontemporal_store(code[0] | (code[1] << 8) | (code[2] << 16) | (code[3] << 24), reinterpret_cast<uint32_t *>(o));
    } else {
#pragma unroll
      for (int c = 0; c < L; ++c)
        if (c < copy) __builtin_nontemporal_store((uint8_t)code[c], o + c);
      for (int c = copy; c < n; ++c) __builtin_nontemporal_store((uint8_t)P.out_fill, o + c);
    }
  } else if (P.out_format == kPackedF16) {
    uint32_t h[L];
#pragma unroll
    for (int c = 0; c < L; ++c) h[c] = c < copy ? (uint32_t)lrp_float_bits_to_half(__float_as_uint(t.v[c])) : (P.out_fill & 0xffffu);
    uint16_t *const o16 = reinterpret_cast<uint16_t *>(o);
    if (P.out_vec) {
      typedef uint32_t v2u __attribute__((ext_vector_type(2)));
      __builtin_nontemporal_store(v2u{h[0] | (h[1] << 16), h[2] | (h[3] << 16)}, reinterpret_cast<v2u *>(o));
    } else {
#pragma unroll
      for (int c = 0; c < L; ++c)
        if (c < copy) __builtin_nontemporal_store((uint16_t)h[c], o16 + c);
      for (int c = copy; c < n; ++c) __builtin_nontemporal_store((uint16_t)P.out_fill, o16 + c);
    }
  } else {
    float *const o32 = reinterpret_cast<float *>(o);
    const float fill = __uint_as_float(P.out_fill);
    if (P.out_vec) {
      typedef float v4f __attribute__((ext_vector_type(4)));
      __builtin_nontemporal_store(v4f{0 < copy ? t.v[0] : fill, 1 < copy ? t.v[1] : fill, 2 < copy ? t.v[2] : fill, 3 < copy ? t.v[3] : fill},
                                  reinterpret_cast<v4f *>(o));
    } else {
#pragma unroll
      for (int c = 0; c < L; ++c)
        if (c < copy) __builtin_nontemporal_store(t.v[c], o32 + c);
      for (int c = copy; c < n; ++c) __builtin_nontemporal_store(fill, o32 + c);
    }
  }
}

// GeoRead: the coordinates come from the geometry-cache entry (P.geo_xy) — no lens math; OutLens is kRect by convention and
// InMode says only whether the source wraps (lrp_cells.h geo_read_cell).
template <int OutLens, int InMode, int Interp, int CH, int Fmt, bool GeoRead>
__global__ __launch_bounds__(kPackedThreads) void packed_kernel(const PackedParams P) {
  constexpr bool Loop = (InMode == kInEquirectLoop);
  constexpr int L = texel_lanes<CH>();
  typedef float vf2 __attribute__((ext_vector_type(2)));
  // The tables first: every thread of the workgroup reaches the barrier (the conditions are uniform over the launch).
  __shared__ float lut[256];
  __shared__ float thr[256];
  const bool want_thr = P.out_format == kPackedU8;
  if constexpr (Fmt == kPackedU8) lut[threadIdx.x] = P.decode[threadIdx.x];
  if (want_thr) thr[threadIdx.x] = P.threshold[threadIdx.x];
  if (Fmt == kPackedU8 || want_thr) __syncthreads();

  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kPackedTileW + (int)(threadIdx.x % kPackedTileW);
  const int y = ty * kPackedTileH + (int)(threadIdx.x / kPackedTileW);
  if (x >= P.out_w || y >= P.out_h) return;

  // source_position and sample<> take a KParams.  Q is NOT a complete one: only the fields those two read today are set —
  // src, in_w / in_h, out_w / out_h, channels, ch_count, in_lens / out_lens, has_rot, rot — and every other field (dst, the
  // table pointers, in_focal / out_focal, the geometry-cache and window-kernel fields) is indeterminate.  A change to
  // lrp_device.h that makes either of them read another field has to set it here; the byte-for-byte tests against the chain
  // (tests/test_gpu_packed.py, every cell x sampler) are what notices.
  KParams Q;
  Q.src = static_cast<const float *>(P.src);
  Q.in_w = P.in_w, Q.in_h = P.in_h;
  Q.out_w = P.out_w, Q.out_h = P.out_h;
  Q.channels = 1; // the samplers' element offsets are texel indices (PackedTaps)
  Q.ch_count = P.channels;
  Q.in_lens = P.in_lens, Q.out_lens = P.out_lens;
  Q.has_rot = P.has_rot;
#pragma unroll
  for (int i = 0; i < 9; ++i) Q.rot[i] = P.rot[i];

  const uint32_t px = geo_map_index(x, y, P.out_w);
  Texel<CH> acc;
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = 0.0f;
  auto add_sample = [&](float sx, float sy) {
    Texel<CH> s;
    if (P.in_vec)
      s = sample<Interp, CH, Loop>(Q, sx, sy, PackedTaps<Fmt, true>{lut, (uint32_t)P.in_pitch, P.in_copy});
    else
      s = sample<Interp, CH, Loop>(Q, sx, sy, PackedTaps<Fmt, false>{lut, (uint32_t)P.in_pitch, P.in_copy});
#pragma unroll
    for (int c = 0; c < L; ++c) acc.v[c] += s.v[c]; // src/reproject.cpp:334-336
  };
  if constexpr (GeoRead) {
    const vf2 xy = reinterpret_cast<const vf2 *>(P.geo_xy)[px];
    add_sample(xy.x, xy.y);
  } else {
    // pixel centre in image-centred coordinates (src/reproject.cpp:287-288) and the sub-sample loop of lrp_kernel_impl.h
    const float cx = ((float)x + 0.5f) - (float)P.out_w * 0.5f;
    const float cy = ((float)y + 0.5f) - (float)P.out_h * 0.5f;
    const int ns = P.num_samples;
    const float ns1 = (float)ns + 1.0f;
    for (int ssx = 0; ssx < ns; ++ssx) {
      const float scx = cx + ((float)ssx + 1.0f) / ns1 - 0.5f; // src/reproject.cpp:295
      for (int ssy = 0; ssy < ns; ++ssy) {
        const float scy = cy + ((float)ssy + 1.0f) / ns1 - 0.5f; // src/reproject.cpp:298
        float sx, sy;
        source_position<OutLens, InMode>(Q, scx, scy, sx, sy);
        if (P.geo_mode == 1) reinterpret_cast<vf2 *>(P.geo_xy)[px] = vf2{sx, sy}; // (num_samples == 1) the entry other launches read
        add_sample(sx, sy);
      }
    }
  }
  // src/reproject.cpp:338-341, then the fused post_process on the first min(C, 3) channels (:423-434)
#pragma unroll
  for (int c = 0; c < L; ++c) acc.v[c] = acc.v[c] * P.normalize;
  if (P.has_post) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < P.channels) acc.v[c] = tonemap(acc.v[c], P.exposure, P.reinhard);
  }
  store_packed<CH>(P, thr, px, acc);
}

// The cells of the packed kernel: all 30 (the extension lenses are gated by the caller's validation), per interpolation,
// source format and lane count, in the layout of the compose kernel's table — entry out_lens * kInModes + in_mode.
template <int Interp, int CH, int Fmt, int Cell> constexpr PackedKernelFn packed_cell_entry() {
  if constexpr (is_lens_id(Cell / kInModes))
    return packed_kernel<Cell / kInModes, Cell % kInModes, Interp, CH, Fmt, false>;
  else
    return nullptr;
}
template <int Interp, int CH, int Fmt, int... Cell>
constexpr std::array<PackedKernelFn, kLensIds * kInModes> packed_cell_table(std::integer_sequence<int, Cell...>) {
  return {{packed_cell_entry<Interp, CH, Fmt, Cell>()...}};
}
template <int Interp, int CH, int Fmt> PackedKernelFn packed_cell_kernel(int out_lens, int in_mode, bool geo_read) {
  static constexpr std::array<PackedKernelFn, kLensIds * kInModes> table =
      packed_cell_table<Interp, CH, Fmt>(std::make_integer_sequence<int, kLensIds * kInModes>{});
  if (out_lens < 0 || out_lens >= kLensIds || in_mode < 0 || in_mode >= kInModes) return nullptr;
  if (geo_read) // no lens math: the wrapping source's kernel or the clamped one's
    return in_mode == kInEquirectLoop ? packed_kernel<kRect, kInEquirectLoop, Interp, CH, Fmt, true> : packed_kernel<kRect, kInEquirect, Interp, CH, Fmt, true>;
  return table[out_lens * kInModes + in_mode];
}

// P: as launch_packed (lrp_packed.hip) completed it.
template <int Interp> hipError_t launch_packed_interp(const PackedParams &P, int in_format, int out_lens, int in_mode, hipStream_t stream) {
  if (P.tiles_x <= 0 || P.tiles_y <= 0) return hipSuccess;
  const bool read = P.geo_mode == 2, four = P.channels <= 4;
  PackedKernelFn fn;
  if (in_format == kPackedU8)
    fn = four ? packed_cell_kernel<Interp, 4, kPackedU8>(out_lens, in_mode, read) : packed_cell_kernel<Interp, 0, kPackedU8>(out_lens, in_mode, read);
  else
    fn = four ? packed_cell_kernel<Interp, 4, kPackedF16>(out_lens, in_mode, read) : packed_cell_kernel<Interp, 0, kPackedF16>(out_lens, in_mode, read);
  if (!fn) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(kXcds * xcd_rows(P.tiles_y) * P.tiles_x)), block(kPackedThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

// ... as a bilinear / bicubic unit of units.list compiles it: defined and instantiated by lrp_packed_unit.hip, declared only for the launcher.
template <int Interp> hipError_t launch_packed_unit(const PackedParams &P, int in_format, int out_lens, int in_mode, hipStream_t stream);
} // namespace lrp
