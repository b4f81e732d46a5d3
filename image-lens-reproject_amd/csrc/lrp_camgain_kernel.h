// lrp_camgain_kernel.h — the calibrated-camera compose kernel with one gain per camera (include/lrp.h "exposure matching across
// a camera rig").  Included by one unit per interpolation (lrp_camgain.hip; lrp_camgain_unit.hip twice,
// units.list) so that the three instantiation sets compile in parallel.
//
// Per output pixel: compose_ss_pixel (lrp_compose_pixel.h) as compose_cam_kernel instantiates it (CameraSources,
// IdealTarget<OutLens>), with CameraGainHook below as the per-sample hook: right after sampling, the first min(C, 3) channels
// of s_i are multiplied by g_i — one v_mul_f32 per channel, ahead of the FIRST / MEAN / FEATHER arithmetic.  A kernel and an
// argument block of its own, so that compose_cam_kernel's do not move.  This kernel is launched for the first group of 8
// channels only: the later groups hold no channel below 3 and go through compose_cam_kernel itself.
//
// Mapping (gfx950): compose_cam_kernel's, unchanged; g_i is one more scalar load from the kernarg block.
#pragma once

#include "lrp_camera_kernel.h"
#include "lrp_camgain.h"

namespace lrp {

using CameraGainKernelFn = void (*)(const CameraGainParams);

// The gain of camera i on its sample: colour only (this launch's channel 0 is the image's).  g_i is read where the hook is
// asked for camera i, at the head of the source loop: read at the multiply instead, six kernels allocate one SGPR fewer.
struct CameraGainHook {
  const float (&gain)[kComposeMaxSources];
  struct Apply {
    float g;
    __device__ __forceinline__ void operator()(Texel<0> &s, int ch_count) const {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c < ch_count) s.v[c] = g * s.v[c];
    }
  };
  __device__ __forceinline__ Apply operator()(int i) const { return {gain[i]}; }
};

template <int OutLens, int Interp>
__global__ __launch_bounds__(kComposeThreads) void camgain_kernel(const CameraGainParams G) {
  const CameraParams &P = G.cam;
  int tx, ty;
  if (!xcd_tile(P.tiles_x, P.tiles_y, tx, ty)) return;
  const int x = tx * kComposeTileW + (int)(threadIdx.x % kComposeTileW);
  const int y = ty * kComposeTileH + (int)(threadIdx.x / kComposeTileW);
  if (x >= P.out_w || y >= P.out_h) return;
  compose_ss_pixel<Interp, CameraSources, IdealTarget<OutLens>>(P, x, y, CameraGainHook{G.gain});
}

// The kernels: one per output lens id.
template <int Interp, int... OutLens>
constexpr std::array<CameraGainKernelFn, kLensIds> camgain_kernel_table(std::integer_sequence<int, OutLens...>) {
  return {{camgain_kernel<OutLens, Interp>...}};
}
template <int Interp> CameraGainKernelFn camgain_kernel_of(int out_lens) {
  static constexpr std::array<CameraGainKernelFn, kLensIds> table = camgain_kernel_table<Interp>(std::make_integer_sequence<int, kLensIds>{});
  if (out_lens < 0 || out_lens >= kLensIds) return nullptr;
  return table[out_lens];
}

template <int Interp> hipError_t launch_compose_cameras_gain_interp(CameraGainParams G, int out_lens, hipStream_t stream) {
  return launch_compose_tiles(camgain_kernel_of<Interp>(out_lens), G, G.cam, stream);
}

// ... as a bilinear / bicubic unit of units.list compiles it: defined and instantiated by lrp_camgain_unit.hip, declared only for the launcher.
template <int Interp> hipError_t launch_compose_cameras_gain_unit(const CameraGainParams &G, int out_lens, hipStream_t stream);
} // namespace lrp
