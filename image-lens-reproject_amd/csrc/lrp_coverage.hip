// lrp_coverage.hip — coverage planes (include/lrp.h "coverage"): per output pixel the number of
// sub-samples whose ray the source image recorded, and — on request — the image mask and the alpha channel made of it.
//
// The render kernels reproduce what the reference does with a ray the source never saw: the samplers clamp (a coordinate
// outside the source smears the border texel) and the sources that fold through x / -z render a mirrored ghost of a ray
// behind the camera.  This kernel evaluates the same lens functions as the one-pixel-per-lane kernel (lrp_kernel_impl.h) —
// target_ray, the rotation, ray_to_source of lrp_device.h: source_position() opened up so that the rotated vz is at hand —
// and decides per sub-sample; it reads no image.
//
// Mapping (gfx950): the plane is one byte per pixel, row-major without padding, i.e. one linear array of out_w * out_h
// bytes.  A lane owns one ALIGNED dword of that array — four consecutive pixels, which may continue in the next row — and
// stores it once: a wavefront writes 256 contiguous bytes with one instruction, a 256-lane workgroup 1 KiB.  Only the first
// and the last dword of a plane can be partial (a plane pointer of any alignment, a pixel count that is no multiple of
// four); those go out as byte stores.  The mask and alpha stores go to the pixels' own texels in the image.
// Numbering: workgroup i takes dwords [256 i, 256 i + 256).  The XCD-aware tile numbering of the render kernels exists for
// their READS (neighbouring tiles share source rows in one XCD's L2); this kernel has none, every 128-byte line of the plane
// is written whole by one wavefront (but for the two lines a misaligned plane splits), and the work per pixel does not depend
// on where the pixel lies — so the dispatcher's round-robin over the XCDs is as good as any other order.
//
// The launch block is the KParams of every kernel (cell_kernel<>'s signature, lrp_cells.h) as make_params() fills it; the
// three values of a coverage launch travel in fields that mean nothing to a kernel without a source (launch_coverage):
//   geo_box   the plane (uint8_t *), null: not wanted        has_post   mask_image
//   ch_count  alpha_channel (-1: none)                        dst        the image of the mask / alpha stores
#include <hip/hip_runtime.h>

#include "lrp_cells.h"
#include "lrp_device.h"

namespace lrp {

namespace {

constexpr int kCovThreads = 256;

// The sources that fold a ray through x / -z (ray_to_source): a ray with vz >= 0 lands on the picture's mirrored ghost.
constexpr bool folding_source(int in_mode) { return in_mode != kInEquirect && in_mode != kInEquirectLoop; }

// One sub-sample: covered iff front && in_x && in_y (include/lrp.h).  Comparisons with NaN are false.
template <int OutLens, int InMode>
__device__ __forceinline__ bool sub_sample_covered(const KParams &P, float scx, float scy) {
  float vx, vy, vz;
  target_ray<OutLens>(P.out_lens, (float)P.out_w, (float)P.out_h, scx, scy, vx, vy, vz);
  if (P.has_rot) { // src/reproject.cpp:301-311
    const float nx = P.rot[0] * vx + P.rot[1] * vy + P.rot[2] * vz;
    const float ny = P.rot[3] * vx + P.rot[4] * vy + P.rot[5] * vz;
    const float nz = P.rot[6] * vx + P.rot[7] * vy + P.rot[8] * vz;
    vx = nx;
    vy = ny;
    vz = nz;
  }
  float px, py;
  ray_to_source<InMode>(P.in_lens, (float)P.in_w, (float)P.in_h, vx, vy, vz, px, py);
  const float sx = (px - 0.5f) + (float)P.in_w * 0.5f; // src/reproject.cpp:323-324
  const float sy = (py - 0.5f) + (float)P.in_h * 0.5f;
  bool ok = sy >= -0.5f && sy <= (float)P.in_h - 0.5f;
  if constexpr (InMode == kInEquirectLoop)
    ok = ok && sx == sx; // the wrapping sampler has a texel for every finite x
  else
    ok = ok && sx >= -0.5f && sx <= (float)P.in_w - 0.5f;
  if constexpr (folding_source(InMode)) ok = ok && vz < 0.0f;
  return ok;
}

template <int OutLens, int InMode> __device__ __forceinline__ uint32_t pixel_count(const KParams &P, int x, int y) {
  // pixel centre and sub-sample positions: src/reproject.cpp:287-298, as in lrp_kernel_impl.h
  const float cx = ((float)x + 0.5f) - (float)P.out_w * 0.5f;
  const float cy = ((float)y + 0.5f) - (float)P.out_h * 0.5f;
  const int ns = P.num_samples;
  const float ns1 = (float)ns + 1.0f;
  uint32_t count = 0;
  for (int ssx = 0; ssx < ns; ++ssx) {
    const float scx = cx + ((float)ssx + 1.0f) / ns1 - 0.5f;
    for (int ssy = 0; ssy < ns; ++ssy) {
      const float scy = cy + ((float)ssy + 1.0f) / ns1 - 0.5f;
      count += sub_sample_covered<OutLens, InMode>(P, scx, scy) ? 1u : 0u;
    }
  }
  return count; // <= 15 * 15
}

template <int OutLens, int InMode> __global__ __launch_bounds__(kCovThreads) void coverage_kernel(const KParams P) {
  uint8_t *const plane = reinterpret_cast<uint8_t *>(P.geo_box);
  const bool mask_image = P.has_post != 0;
  const int alpha = P.ch_count, C = P.channels;
  const uint32_t n_px = (uint32_t)P.out_w * (uint32_t)P.out_h; // <= 2^31 (launch_coverage's caller)
  // pixel i is byte plane + i: the dword of this lane holds pixels base - off .. base - off + 3
  const uint32_t off = (uint32_t)(reinterpret_cast<uintptr_t>(plane) & 3u);
  const uint32_t base = (blockIdx.x * (uint32_t)kCovThreads + threadIdx.x) * 4u;
  const uint32_t first = base >= off ? base - off : 0u; // first pixel of this lane (the plane's first dword: its valid tail)
  if (first >= n_px) return;
  const uint32_t n_here = min(base + 4u - off, n_px) - first; // 1 .. 4
  int y = (int)(first / (uint32_t)P.out_w), x = (int)(first - (uint32_t)y * (uint32_t)P.out_w);
  uint32_t packed = 0;
#pragma unroll 1 // (one copy of the lens math per kernel: four cost registers and code size and buy nothing)
  for (uint32_t j = 0; j < n_here; ++j) {
    const uint32_t i = first + j;
    const uint32_t count = pixel_count<OutLens, InMode>(P, x, y);
    packed |= count << (8u * j);
    if (mask_image && count == 0u) { // every channel +0.0f; a covered pixel keeps its bytes
      float *const t = P.dst + (size_t)i * (size_t)C;
      for (int c = 0; c < C; ++c) t[c] = 0.0f;
    }
    if (alpha >= 0) P.dst[(size_t)i * (size_t)C + (size_t)alpha] = (float)count * P.normalize; // every pixel, behind the mask
    if (++x == P.out_w) {
      x = 0;
      ++y;
    }
  }
  if (plane == nullptr) return;
  if (n_here == 4u) { // (then first == base - off: plane + first is the aligned dword)
    __builtin_nontemporal_store(packed, reinterpret_cast<uint32_t *>(plane + first));
  } else {
    for (uint32_t j = 0; j < n_here; ++j) plane[first + j] = (uint8_t)(packed >> (8u * j));
  }
}

// The cells of the coverage kernel: all of them, in this one unit (the extension lenses are gated by the caller's validation).
struct CoverageCell {
  template <int OutLens, int InMode> static constexpr KernelFn kernel() { return coverage_kernel<OutLens, InMode>; }
};

} // namespace

// P: make_params() of the call (lenses, sizes, rotation, num_samples, normalize; dst = the image or null).
hipError_t launch_coverage(KParams P, int out_lens, int in_mode, uint8_t *plane, int mask_image, int alpha_channel, hipStream_t stream) {
  P.src = nullptr;
  P.geo_box = reinterpret_cast<int32_t *>(plane);
  P.has_post = mask_image != 0;
  P.ch_count = alpha_channel;
  const KernelFn fn = cell_kernel<CoverageCell>(out_lens, in_mode);
  if (!fn) return hipErrorInvalidValue;
  const unsigned long long n_px = (unsigned long long)P.out_w * (unsigned long long)P.out_h;
  const unsigned long long dwords = (n_px + (reinterpret_cast<uintptr_t>(plane) & 3u) + 3u) / 4u;
  const dim3 grid((unsigned)((dwords + kCovThreads - 1) / kCovThreads)), block(kCovThreads);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace lrp
