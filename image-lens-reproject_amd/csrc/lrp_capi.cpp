// lrp_capi.cpp — the C ABI declared in include/lrp.h: argument validation in the
// reference's dispatch order, kernel-argument construction, device buffers,
// streams and the batch context.  Host code only; the kernels live in the
// lrp_kernels_*.hip / lrp_tile_*.hip / lrp_{pixel,tile,win}_unit.hip (reprojection), lrp_tables.hip, lrp_geo_lists.hip,
// lrp_coverage.hip (coverage planes), lrp_compose*.hip (compose), lrp_camera*.hip (compose, calibrated cameras), lrp_camview*.hip (a calibrated camera as the target), lrp_packed*.hip (packed pixels), lrp_lanczos*.hip (the Lanczos-3 sampler), lrp_pixel_kernels.hip and lrp_aux_kernels.hip translation units; units.list names every object and what it is compiled from.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/lrp.h"
#include "lrp_camera.h"
#include "lrp_camera_inverse.h"
#include "lrp_camera_packed.h"
#include "lrp_camgain.h"
#include "lrp_camstat.h"
#include "lrp_camview.h"
#include "lrp_compose.h"
#include "lrp_compose_packed.h"
#include "lrp_compose_ss.h"
#include "lrp_geocache.h"
#include "lrp_mb_packed.h"
#include "lrp_multiband.h"
#include "lrp_packed.h"
#include "lrp_params.h"
#include "lrp_plan.h"
#include "lrp_tables.h"

namespace lrp {
// out_lens / in_mode: the ids of lrp_params.h, for every lens (lrp_cells.h)
hipError_t launch_nearest(const KParams &P, int out_lens, int in_mode, hipStream_t stream);
hipError_t launch_bilinear(const KParams &P, int out_lens, int in_mode, hipStream_t stream);
hipError_t launch_bicubic(const KParams &P, int out_lens, int in_mode, hipStream_t stream);
hipError_t launch_tile_nearest(const KParams &P, int out_lens, int in_mode, hipStream_t stream);
hipError_t launch_tile_bilinear(const KParams &P, int out_lens, int in_mode, hipStream_t stream);
hipError_t launch_tile_bicubic(const KParams &P, int out_lens, int in_mode, hipStream_t stream);
hipError_t launch_win_bicubic(const KParams &P, int out_lens, int in_mode, hipStream_t stream); // (P.geo_mode == 2: the GeoRead kernels)
hipError_t launch_ss_gather(const KParams &P, int interpolation, int in_mode, hipStream_t stream); // lrp_tile_ssg.hip: nearest / bilinear, num_samples 2-4, from an entry of sub-samples
hipError_t launch_geo_build_lists(int32_t *box, int out_w, int out_h, int alias_pairs, hipStream_t stream); // lrp_geo_lists.hip
hipError_t launch_geo_census(int32_t *box, int out_w, int out_h, int in_w, int in_h, bool clear_header, hipStream_t stream); // lrp_geo_lists.hip
hipError_t launch_corner_fill(const KParams &P, hipStream_t stream);
// lrp_coverage.hip.  A weak reference: the host-code test drivers (tests/native/multi_driver.cpp) link this file against stand-ins
// of the launchers they exercise; where the unit is not linked in, a coverage request fails (enqueue_coverage).
__attribute__((weak)) hipError_t launch_coverage(KParams P, int out_lens, int in_mode, uint8_t *plane, int mask_image, int alpha_channel, hipStream_t stream);
// lrp_compose.hip, weak like launch_coverage (enqueue_compose).
__attribute__((weak)) hipError_t launch_compose(const ComposeParams &P, int out_lens, int in_mode, int interpolation, hipStream_t stream);
// lrp_compose_ss.hip, weak like launch_compose (enqueue_compose_ss).
__attribute__((weak)) hipError_t launch_compose_ss(const ComposeSsParams &P, int out_lens, int in_mode, int interpolation, hipStream_t stream);
// lrp_camera.hip, weak like launch_compose (enqueue_compose_cameras).
__attribute__((weak)) hipError_t launch_compose_cameras(const CameraParams &P, int out_lens, int interpolation, hipStream_t stream);
// lrp_camview.hip, weak likewise (enqueue_camera_view).
__attribute__((weak)) hipError_t launch_camera_view(const CameraViewParams &P, int interpolation, hipStream_t stream);
// lrp_camstat.hip and lrp_camgain.hip, weak likewise (enqueue_camera_overlap, enqueue_compose_cameras_gain).
__attribute__((weak)) hipError_t launch_camera_overlap(const CameraStatParams &P, int out_lens, hipStream_t stream);
__attribute__((weak)) hipError_t launch_compose_cameras_gain(const CameraGainParams &G, int out_lens, int interpolation, hipStream_t stream);
// lrp_multiband_label.hip and lrp_multiband.hip, weak likewise (enqueue_multiband).
__attribute__((weak)) hipError_t launch_multiband_label(const MultibandLabelParams &P, int out_lens, hipStream_t stream);
__attribute__((weak)) hipError_t launch_multiband_reduce(const MultibandReduceParams &P, int channels, hipStream_t stream);
__attribute__((weak)) hipError_t launch_multiband_lap(const MultibandLapParams &P, int channels, hipStream_t stream);
__attribute__((weak)) hipError_t launch_multiband_collapse(const MultibandCollapseParams &P, int channels, hipStream_t stream);
// lrp_packed.hip, weak like launch_coverage (enqueue_packed).
__attribute__((weak)) hipError_t launch_packed(PackedParams P, int in_format, int out_lens, int in_mode, int interpolation, int device, hipStream_t stream);
// lrp_compose_packed.hip, weak like launch_coverage (enqueue_compose_packed).
__attribute__((weak)) hipError_t launch_compose_packed(ComposePackedParams P, int in_format, int out_lens, int in_mode, int interpolation, int device, hipStream_t stream);
// lrp_camera_packed.hip and lrp_camstat_packed.hip, weak likewise (enqueue_compose_cameras_packed, enqueue_camera_overlap_packed).
__attribute__((weak)) hipError_t launch_compose_cameras_packed(CameraPackedParams P, int in_format, int out_lens, int interpolation, int device, hipStream_t stream);
__attribute__((weak)) hipError_t launch_camera_overlap_packed(CameraStatPackedParams P, int in_format, int out_lens, int device, hipStream_t stream);
// lrp_mb_packed.hip, weak likewise (enqueue_multiband with a packed side).
__attribute__((weak)) hipError_t launch_mb_collapse_packed(MbCollapsePackedParams P, int channels, int device, hipStream_t stream);
// lrp_lanczos.hip, weak like launch_coverage (enqueue_lanczos).
__attribute__((weak)) hipError_t launch_lanczos(KParams P, int out_lens, int in_mode, hipStream_t stream);
hipError_t launch_post_process(float *data, uint32_t n_pixels, int channels, float exposure, float reinhard,
                               hipStream_t stream);
hipError_t launch_synth_fill(float *data, uint32_t n_elems, int channels, uint32_t seed, int depth_channel,
                             hipStream_t stream);
hipError_t launch_math_eval(int func, const float *a, const float *b, float *out, size_t n, hipStream_t stream);
hipError_t launch_checksum(const float *data, size_t n, unsigned long long *out, hipStream_t stream);
size_t pixel_bytes(int format, int channels);
hipError_t launch_decode_pixels(const void *src, int format, int src_channels, float *dst, int dst_channels,
                                size_t n_pixels, int device, hipStream_t stream);
hipError_t launch_encode_pixels(const float *src, int src_channels, void *dst, int format, int dst_channels,
                                unsigned fill, size_t n_pixels, int device, hipStream_t stream);
void pixel_tables_host(float decode[256], float threshold[256]);
} // namespace lrp

namespace {

thread_local std::string g_last_error;

int fail(int status, const std::string &detail) {
  g_last_error = detail;
  return status;
}

int hip_fail(hipError_t e, const char *what) {
  int st = (e == hipErrorOutOfMemory) ? LRP_ERR_OOM : LRP_ERR_HIP;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) st = LRP_ERR_NO_DEVICE;
  return fail(st, std::string(what) + ": " + hipGetErrorString(e));
}

#define LRP_HIP_TRY(expr)                                                                                    \
  do {                                                                                                       \
    hipError_t _e = (expr);                                                                                  \
    if (_e != hipSuccess) return hip_fail(_e, #expr);                                                        \
  } while (0)

int device_count_cached() {
  static int count = [] {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    return n < 0 ? 0 : n;
  }();
  return count;
}

int select_device(int device) {
  const int n = device_count_cached();
  if (n == 0) return fail(LRP_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU path");
  if (device < 0 || device >= n) return fail(LRP_ERR_NO_DEVICE, "device index out of range");
  LRP_HIP_TRY(hipSetDevice(device));
  return LRP_OK;
}

// Opt-in lens extensions (lrp_lens_extensions): a mask of LRP_LENS_EXT_*, 0 — the reference's lenses only — by default.
std::atomic<int> g_lens_ext{0};

// Opt-in sampler extensions (lrp_sampler_extensions): a mask of LRP_SAMPLER_EXT_*, 0 — the reference's samplers only — by default.
std::atomic<int> g_sampler_ext{0};

// `ext`: the extension mask, read once per call
bool lens_in_hot_path(int type, int ext) {
  return type == LRP_RECTILINEAR || type == LRP_FISHEYE_EQUIDISTANT || type == LRP_EQUIRECTANGULAR ||
         (type == LRP_FISHEYE_EQUISOLID && (ext & LRP_LENS_EXT_EQUISOLID) != 0) ||
         (type == LRP_FISHEYE_STEREOGRAPHIC && (ext & LRP_LENS_EXT_STEREOGRAPHIC) != 0);
}

// LoopHorizontally decision, reference src/reproject.cpp:386-394: float span,
// compared in double against 2*M_PI with a float threshold.
bool source_wraps(const lrp_lens &L) {
  const float long_range = L.u.equirectangular.longitude_max - L.u.equirectangular.longitude_min;
  return std::fabs((double)long_range - (2 * M_PI)) < 1e-5f;
}

int in_lens_mode(const lrp_lens &L) {
  if (L.type == LRP_RECTILINEAR) return lrp::kInRect;
  if (L.type == LRP_FISHEYE_EQUIDISTANT) return lrp::kInEquidistant;
  if (L.type == LRP_FISHEYE_EQUISOLID) return lrp::kInEquisolid;
  if (L.type == LRP_FISHEYE_STEREOGRAPHIC) return lrp::kInStereographic;
  return source_wraps(L) ? lrp::kInEquirectLoop : lrp::kInEquirect;
}

lrp::LensP pack_lens(const lrp_lens &L) {
  lrp::LensP p;
  std::memcpy(p.p, L.u.raw, sizeof(p.p));
  p.sensor_width = L.sensor_width;
  p.sensor_height = L.sensor_height;
  return p;
}

size_t image_bytes(const lrp_image &im) { return (size_t)im.width * (size_t)im.height * (size_t)im.channels * 4u; }
// The reference addresses texels with `int` (src/reproject.cpp:49-51,134-142: ly * pitch + lx * channels + c): an image of
// up to 2^31 floats (8 GiB) is what it can render; beyond that its index overflows.  Same limit here.
constexpr unsigned long long kMaxImageFloats = 1ull << 31;
bool image_addressable(const lrp_image &im) {
  return (unsigned long long)im.width * (unsigned long long)im.height * (unsigned long long)im.channels <= kMaxImageFloats;
}
// The tile / window kernels address texels through 32-bit byte offsets (buffer descriptors, LDS-DMA): images below 4 GiB.
// Larger ones — [4 GiB, 8 GiB] — take the one-pixel-per-lane kernel, whose element offsets are 32-bit and pointers 64-bit.
bool image_fits_byte_offsets(const lrp_image &im) { return (unsigned long long)image_bytes(im) < (1ull << 32); }

// Checks in the order the reference dispatches: output lens
// (src/reproject.cpp:408-418), input lens (:378-398), interpolation (:352-367);
// then the preconditions the reference leaves unchecked.  lanczos_entry: the entry point renders LRP_LANCZOS3 while
// LRP_SAMPLER_EXT_LANCZOS3 is on (every one that reaches enqueue_reproject; compose and packed pixels do not).
int validate(const lrp_image *in, const lrp_image *out, int interpolation, bool need_data, bool lanczos_entry) {
  if (!in || !out) return fail(LRP_ERR_NULL, "null image");
  const int ext = g_lens_ext.load(std::memory_order_relaxed);
  if (!lens_in_hot_path(out->lens.type, ext)) return fail(LRP_ERR_OUTPUT_LENS, "Output lens type not supported.");
  if (!lens_in_hot_path(in->lens.type, ext)) return fail(LRP_ERR_INPUT_LENS, "Input lens type not supported.");
  const bool lanczos = interpolation == LRP_LANCZOS3 && lanczos_entry && (g_sampler_ext.load(std::memory_order_relaxed) & LRP_SAMPLER_EXT_LANCZOS3) != 0;
  if (interpolation != LRP_NEAREST && interpolation != LRP_BILINEAR && interpolation != LRP_BICUBIC && !lanczos)
    return fail(LRP_ERR_INTERPOLATION, "Interpolation method not supported.");
  if (in->channels < 1 || in->channels != out->channels)
    return fail(LRP_ERR_CHANNELS, "in->channels must equal out->channels and be >= 1");
  if (in->width < 1 || in->height < 1 || out->width < 1 || out->height < 1)
    return fail(LRP_ERR_BAD_DIMS, "image dimensions must be positive");
  if (!image_addressable(*in) || !image_addressable(*out))
    return fail(LRP_ERR_BAD_DIMS, "an image of more than 2^31 floats (8 GiB) cannot be addressed (the reference indexes texels with int, src/reproject.cpp:49-51)");
  if (need_data && (!in->data || !out->data)) return fail(LRP_ERR_NULL, "null image data");
  return LRP_OK;
}

lrp::KParams make_params(const lrp_image *in, const lrp_image *out, int num_samples, const float *rotation,
                         const lrp_post *post) {
  lrp::KParams P;
  std::memset(&P, 0, sizeof(P));
  P.src = in->data;
  P.dst = out->data;
  P.in_w = in->width;
  P.in_h = in->height;
  P.out_w = out->width;
  P.out_h = out->height;
  P.channels = out->channels;
  P.ch_count = out->channels;
  P.num_samples = num_samples;
  P.normalize = 1.0f / (float)(num_samples * num_samples); // src/reproject.cpp:280
  P.in_lens = pack_lens(in->lens);
  P.out_lens = pack_lens(out->lens);
  P.has_rot = rotation != nullptr;
  if (rotation) std::memcpy(P.rot, rotation, sizeof(P.rot));
  P.has_post = post != nullptr;
  if (post) {
    P.exposure = post->exposure;
    P.reinhard = post->reinhard;
  }
  P.y_offset = 0;
  P.y_end = out->height;
  // lens-only constants of the tile kernel, same binary32 operations as the
  // reference performs per pixel (src/reproject.cpp:178,196,265-266)
  P.in_focal = in->lens.sensor_width / in->lens.u.fisheye_equidistant.fov;
  P.out_focal = out->lens.sensor_width / out->lens.u.fisheye_equidistant.fov;
  // equisolid: 2.0f * focal_length, exact (r = 2 f sin(theta / 2), include/lrp.h)
  if (in->lens.type == LRP_FISHEYE_EQUISOLID) P.in_focal = 2.0f * in->lens.u.fisheye_equisolid.focal_length;
  if (out->lens.type == LRP_FISHEYE_EQUISOLID) P.out_focal = 2.0f * out->lens.u.fisheye_equisolid.focal_length;
  // stereographic: likewise (r = 2 f tan(theta / 2))
  if (in->lens.type == LRP_FISHEYE_STEREOGRAPHIC) P.in_focal = 2.0f * in->lens.u.fisheye_stereographic.focal_length;
  if (out->lens.type == LRP_FISHEYE_STEREOGRAPHIC) P.out_focal = 2.0f * out->lens.u.fisheye_stereographic.focal_length;
  P.in_lon_span = in->lens.u.equirectangular.longitude_max - in->lens.u.equirectangular.longitude_min;
  P.in_lat_span = in->lens.u.equirectangular.latitude_max - in->lens.u.equirectangular.latitude_min;
  return P;
}

// Kernel selection and the A/B switches of the sharing / staging paths.  All of them live in one table of atomics that
// lrp_debug_set() reads and writes (tests, tools/policy_check.py); the library reads no environment variable.
//   kernel: 0 = pixel kernel, 1 = tile kernel everywhere, 2 (default) = tile kernel with the LDS-window kernel for
//   bicubic, 3 = the same without its shared-coefficient tier and without any work sharing.  All HIP; there is no CPU path.
enum DebugKnob : int { kKnobKernel = 0, kKnobXsep, kKnobQuad, kKnobMirrorModes, kKnobWinEdge, kKnobWinSplit, kKnobBatchFrames, kKnobMultiFork, kKnobGeoCache, kKnobGeoStrip, kKnobGeoBig, kKnobGeoLists, kKnobGeoFillStream, kKnobGeoFillFused, kKnobContextStreams, kKnobWinTapDma, kKnobGeoCensus, kKnobGeoListRecs, kKnobWinSS, kKnobListedLaunches, kKnobBigLaunches, kKnobCount };
struct KnobSpec {
  const char *name;
  int lo, hi, initial;
};
constexpr int kMaxSideStreams = 5;
const KnobSpec kKnobs[kKnobCount] = {
    {"kernel", 0, 3, 2},
    {"xsep", 0, 1, 1},                  // column-separable source x tables
    {"quad", 0, 1, 1},                  // mirrored pixels / blocks (every mirror mode)
    {"mirror_modes", 0, 1, 1},  // window kernel: pan / pitch / shared-ray mirror modes
    {"win_edge", 0, 1, 1},          // window kernel: blocks beyond one side of the source stage one row / column
    {"win_split", 0, 1, 1},        // window kernel: split blocks and pass windows
    {"batch_frames", 0, lrp::kMaxBatch, 0}, // frames per wavefront of a batched launch (0: automatic); > 1 on a launch that reads the geometry cache: one block per wavefront, whatever geo_strip says
    {"multi_fork", 0, kMaxSideStreams, 1},    // side streams of lrp_reproject_multi_device
    {"geo_cache", 0, 1, 1},        // geometry cache used by single launches (0: every launch computes)
    {"geo_strip", 0, lrp::kGeoStripRows, 0}, // blocks per wavefront of a launch that reads the geometry cache (0: automatic); launches without the frame loop only
    {"geo_big", 0, 2, 1},            // big-window variant of the kernels that read the geometry cache (a rectilinear view rendered into a panorama); 0: the four-wavefront instantiation
    {"geo_lists", 0, 2, 1},        // rendering by block class from the lists of a geometry-cache entry (corner runs by the fill kernel / a share per wavefront, the window kernel over the work list): 0 never, 1 where at least 30 % of the blocks are corner blocks, 2 whenever the lists are known
    {"geo_fill_stream", 0, 1, 0}, // the fill kernel of a listed launch: 0 in front of the window kernel on the caller's stream, 1 beside it on a side stream of the device
    {"geo_fill_fused", 0, 1, 1}, // the corner runs of a listed launch as a share per wavefront of the window kernel (0: always the fill kernel)
    {"context_streams", 0, 1, 1}, // lrp_context: consecutive images alternate between two compute streams (0: one)
    {"win_tapdma", 0, 1, 1},      // window kernel: passes whose window fits no buffer fetch their taps a quad of lanes per pixel row through LDS-DMA (0: a gather per lane and tap)
    {"geo_census", 0, 1, 1},      // the census of a new geometry-cache entry's windows (lrp_geo_lists.hip; what the automatic choice of the big-window variant reads); 0: not taken
    {"geo_list_recs", 0, 1, 1}, // listed launches: a wavefront reads its block's box record from beside its work-list entry, with the entry (0: from the box array, a second round trip)
    {"win_ss", 0, 1, 1},              // bicubic with num_samples 2-4 through the window kernel's supersampling instantiations (0: the tile kernel, as for any other num_samples > 1)
    {"listed_launches", 0, 0, 0}, // a counter, not a switch: launches rendered by block class so far (set 0 to reset; tests, bench)
    {"big_launches", 0, 0, 0},       // a counter: window launches through the big-window variant so far
};
std::atomic<int> g_knobs[kKnobCount];
const bool g_knobs_initialised = [] {
  for (int k = 0; k < kKnobCount; ++k) g_knobs[k].store(kKnobs[k].initial, std::memory_order_relaxed);
  return true;
}();
int knob(int k) { return g_knobs[k].load(std::memory_order_relaxed); }
int kernel_choice() { return knob(kKnobKernel); }

// The fill kernel of a listed launch (lrp_geo_lists.hip).  In front of the window kernel on the caller's stream, or — knob
// "geo_fill_stream" — beside it on a side stream of the device: the two write disjoint pixels, the window kernel holds
// two to four wavefronts per SIMD and all of a CU's LDS, the fill kernel needs neither.  Fork / join by events, so the
// caller's stream order is kept; not while that stream is being captured.
struct FillFork {
  std::mutex busy; // one fork / join being enqueued at a time per device (the events are re-recorded by every call)
  hipStream_t side = nullptr;
  hipEvent_t forked = nullptr, joined = nullptr;
};
std::mutex g_fill_fork_mutex;
std::map<int, std::unique_ptr<FillFork>> g_fill_forks;
FillFork *fill_fork(int device) {
  std::lock_guard<std::mutex> lock(g_fill_fork_mutex);
  std::unique_ptr<FillFork> &slot = g_fill_forks[device];
  if (!slot) {
    std::unique_ptr<FillFork> f(new FillFork);
    if (hipStreamCreateWithFlags(&f->side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&f->forked, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&f->joined, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    slot = std::move(f);
  }
  return slot.get();
}
hipError_t fill_corner_runs(const lrp::KParams &P, int device, hipStream_t stream) {
  if (P.geo_n_runs == 0) return hipSuccess;
  if (knob(kKnobGeoFillStream) != 0) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) (void)hipGetLastError();
    FillFork *const f = cap == hipStreamCaptureStatusNone ? fill_fork(device) : nullptr;
    if (f != nullptr) {
      std::lock_guard<std::mutex> lock(f->busy);
      if (hipEventRecord(f->forked, stream) == hipSuccess && hipStreamWaitEvent(f->side, f->forked, 0) == hipSuccess) {
        const hipError_t e = lrp::launch_corner_fill(P, f->side);
        // join, whatever happened: the caller's stream continues behind the side stream
        if (hipEventRecord(f->joined, f->side) != hipSuccess || hipStreamWaitEvent(stream, f->joined, 0) != hipSuccess) {
          (void)hipGetLastError();
          (void)hipStreamSynchronize(f->side);
        }
        return e;
      }
      (void)hipGetLastError();
    }
  }
  return lrp::launch_corner_fill(P, stream);
}

// n_batch > 0: `in` / `out` are arrays of n_batch images of one geometry (checked by the caller);
// the tile / window kernels render them in launches of up to kMaxBatch frames, the per-pixel
// kernels one launch per frame.
// row_count > 0: only output rows [row_first, row_first + row_count) are rendered (the rows of the reference
// loop are independent, src/reproject.cpp:284); the kernels that share work between mirrored rows need the
// whole image and are not used for a band.
// The switches the planner reads, at their current values.
lrp::PlanSwitches plan_switches() {
  lrp::PlanSwitches s;
  s.kernel = kernel_choice();
  s.xsep = knob(kKnobXsep), s.quad = knob(kKnobQuad), s.mirror_modes = knob(kKnobMirrorModes);
  s.win_edge = knob(kKnobWinEdge), s.win_split = knob(kKnobWinSplit), s.win_tapdma = knob(kKnobWinTapDma), s.win_ss = knob(kKnobWinSS);
  s.batch_frames = knob(kKnobBatchFrames);
  s.geo_cache = knob(kKnobGeoCache), s.geo_strip = knob(kKnobGeoStrip), s.geo_big = knob(kKnobGeoBig), s.geo_lists = knob(kKnobGeoLists);
  s.geo_fill_fused = knob(kKnobGeoFillFused), s.geo_list_recs = knob(kKnobGeoListRecs);
  return s;
}

lrp::PlanRequest plan_request(const lrp_image *in, const lrp_image *out, int num_samples, int interpolation, const float *rotation,
                              int n_batch, bool band) {
  lrp::PlanRequest r;
  r.out_type = out->lens.type; // (the lens ids of lrp_params.h are the numbering of include/lrp.h: asserted below)
  r.in_type = in->lens.type;
  r.in_mode = in_lens_mode(in->lens);
  r.out_w = out->width, r.out_h = out->height, r.in_w = in->width, r.in_h = in->height, r.channels = out->channels;
  r.num_samples = num_samples, r.interpolation = interpolation;
  r.has_rot = rotation != nullptr;
  if (rotation) std::memcpy(r.rot, rotation, sizeof(r.rot));
  r.out_lon_span = out->lens.u.equirectangular.longitude_max - out->lens.u.equirectangular.longitude_min;
  r.n_batch = n_batch;
  r.band = band;
  r.byte_offsets_fit = image_fits_byte_offsets(*in) && image_fits_byte_offsets(*out);
  return r;
}
static_assert((int)lrp::kPlanRect == (int)lrp::kRect && (int)lrp::kPlanEquidistant == (int)lrp::kEquidistant && (int)lrp::kPlanEquirect == (int)lrp::kEquirect &&
                  (int)lrp::kPlanEquisolid == (int)lrp::kEquisolid && (int)lrp::kPlanStereographic == (int)lrp::kStereographic,
              "lrp_plan.h numbers lenses like lrp_params.h");
static_assert((int)lrp::kRect == LRP_RECTILINEAR && (int)lrp::kEquidistant == LRP_FISHEYE_EQUIDISTANT && (int)lrp::kEquisolid == LRP_FISHEYE_EQUISOLID &&
                  (int)lrp::kStereographic == LRP_FISHEYE_STEREOGRAPHIC && (int)lrp::kEquirect == LRP_EQUIRECTANGULAR,
              "lrp_params.h numbers lenses like include/lrp.h");
static_assert((int)lrp::kPlanInRect == (int)lrp::kInRect && (int)lrp::kPlanInEquidistant == (int)lrp::kInEquidistant &&
                  (int)lrp::kPlanInEquirect == (int)lrp::kInEquirect && (int)lrp::kPlanInEquirectLoop == (int)lrp::kInEquirectLoop &&
                  (int)lrp::kPlanInEquisolid == (int)lrp::kInEquisolid && (int)lrp::kPlanInStereographic == (int)lrp::kInStereographic,
              "lrp_plan.h numbers input modes like lrp_params.h");
static_assert((int)lrp::kPlanNearest == LRP_NEAREST && (int)lrp::kPlanBilinear == LRP_BILINEAR && (int)lrp::kPlanBicubic == LRP_BICUBIC, "interpolation numbering");

// The geometry-cache key of a call: everything the coordinates depend on (lrp_geocache.h).
lrp::GeoKey geo_key(const lrp_image *in, const lrp_image *out, const lrp::KParams &P, int num_samples, int device) {
  lrp::GeoKey key;
  std::memset(&key, 0, sizeof(key));
  key.device = device;
  key.out_type = out->lens.type;
  key.in_mode = in_lens_mode(in->lens);
  key.out_w = out->width, key.out_h = out->height, key.in_w = in->width, key.in_h = in->height;
  key.has_rot = P.has_rot;
  key.num_samples = num_samples;
  key.out_lens = lrp::geo_canonical_lens(P.out_lens, out->lens.type), key.in_lens = lrp::geo_canonical_lens(P.in_lens, in->lens.type);
  if (P.has_rot) std::memcpy(key.rot, P.rot, sizeof(key.rot));
  return key;
}

// LRP_LANCZOS3 (include/lrp.h "Lanczos-3"; lrp_lanczos.hip): the planner is not asked — one kernel shape, one launch per frame
// and per group of 8 channels (RGBA: one group of 4) on the caller's stream, like the pixel-kernel branch of enqueue_reproject.
// num_samples == 1, whole images, "geo_cache" on: through the geometry cache under the key of every other sampler for this
// geometry, as enqueue_packed does — the first launch writes the coordinate map as a side output, every later launch (of the
// call, or of any sampler) loads it.  No allocation, no synchronisation and no lens table on this path.
int enqueue_lanczos(const lrp_image *in, lrp_image *out, lrp::KParams P, const lrp_post *post, int device, hipStream_t stream, int n_batch, bool band) {
  if (!lrp::launch_lanczos) return fail(LRP_ERR_HIP, "the Lanczos-3 kernels (lrp_lanczos.hip) are not part of this build");
  const int ol = out->lens.type, im = in_lens_mode(in->lens);
  lrp::GeoUse geo;
  if (P.num_samples == 1 && !band && knob(kKnobGeoCache) != 0) {
    lrp::geo_acquire(geo_key(in, out, P, P.num_samples, device), /*want_boxes=*/false, stream, &geo);
    if (geo.mode == 1 || geo.mode == 2) {
      P.geo_mode = geo.mode;
      P.geo_xy = geo.xy;
    }
  }
  const int n = n_batch > 0 ? n_batch : 1;
  const int C = out->channels, group = C == 4 ? 4 : 8;
  hipError_t e = hipSuccess;
  for (int i = 0; i < n && e == hipSuccess; ++i)
    for (int c0 = 0; c0 < C && e == hipSuccess; c0 += group) {
      P.src = in[i].data + c0;
      P.dst = out[i].data + c0;
      P.ch_count = std::min(group, C - c0);
      P.has_post = post != nullptr && c0 == 0; // post_process touches channels 0-2 only: all in the first group
      e = lrp::launch_lanczos(P, ol, im, stream);
      if (P.geo_mode == 1) P.geo_mode = 2; // the launch that writes the entry goes first; the rest follows on the same stream and reads it
    }
  lrp::geo_launched(&geo, stream, e == hipSuccess);
  if (e != hipSuccess) return hip_fail(e, "Lanczos-3 kernel launch");
  return LRP_OK;
}

// The launcher: asks the planner (lrp_plan.h — every decision is there, as pure functions the CPU tests call too), fetches what
// the plan wants (output-lens tables, the column-separable x table, the geometry-cache entry) and enqueues the launches.
int enqueue_reproject(const lrp_image *in, lrp_image *out, int num_samples, int interpolation,
                      const float *rotation, const lrp_post *post, int device, hipStream_t stream, int n_batch = 0,
                      int row_first = 0, int row_count = 0) {
  if (num_samples <= 0) return LRP_OK; // reference loop body never runs: output untouched
  lrp::KParams P = make_params(in, out, num_samples, rotation, post);
  const bool band = row_count > 0 && !(row_first == 0 && row_count == out->height);
  if (band) {
    P.y_offset = row_first;
    P.y_end = row_first + row_count;
  }
  if (interpolation == LRP_LANCZOS3) return enqueue_lanczos(in, out, P, post, device, stream, n_batch, band);
  const int ol = out->lens.type, im = in_lens_mode(in->lens); // the cell of this call (lrp_cells.h)
  hipError_t e;
  lrp::TableLease lease; // pins the cached tables until every launch of this call is enqueued (scope end)
  lrp::GeoUse geo;       // this launch's use of the geometry cache (none unless set below)
  const lrp::PlanSwitches sw = plan_switches();
  const lrp::PlanRequest req = plan_request(in, out, num_samples, interpolation, rotation, n_batch, band);
  lrp::PlanFamily family = lrp::plan_family(req, sw);
  lrp::TableFacts tables;
  if (family.wants_tables) {
    // separable output-lens terms (cached per device / lens / size / num_samples)
    const int out_kind = out->lens.type == LRP_RECTILINEAR ? lrp::kRect : lrp::kEquirect;
    e = lrp::get_output_tables(device, out_kind, P.out_lens, out->width, out->height, num_samples, stream, lease,
                               &P.col_tab, &P.row_tab, &tables.plain, &tables.symmetry);
    if (e == hipErrorOutOfMemory) { // the geometry cache of THIS GPU holds what it holds for speed only: give it back, once
      (void)hipGetLastError();
      lrp::geo_release_device(device);
      e = lrp::get_output_tables(device, out_kind, P.out_lens, out->width, out->height, num_samples, stream, lease,
                                 &P.col_tab, &P.row_tab, &tables.plain, &tables.symmetry);
    }
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      family.tile = false; // no memory for the tables: per-pixel kernel
    } else if (e != hipSuccess) {
      return hip_fail(e, "output-lens table build");
    } else {
      tables.built = true;
      const lrp::PlanRotation pr = lrp::plan_rotation(req, sw, family, tables);
      P.has_rot = pr.has_rot ? 1 : 0;
      if (pr.wants_xsep)
        P.xsep_tab = lrp::get_xsep_table(device, P.col_tab, out_kind, out->width, num_samples, P.in_lens, im, in->width,
                                         P.in_lon_span, P.has_rot ? P.rot : nullptr, stream, lease);
    }
  }
  if (family.tile) {
    lrp::PlanRotation pr;
    pr.has_rot = P.has_rot != 0;
    const lrp::PlanSharing sh = lrp::plan_sharing(req, sw, family, tables, pr, P.xsep_tab != nullptr);
    const bool window = sh.window;
    P.quad = sh.quad;
    P.win_coef = sh.win_coef, P.win_edge = sh.win_edge, P.win_split = sh.win_split, P.win_tapdma = sh.win_tapdma;
    P.win_mode = sh.win_mode;
    P.alias_pairs = sh.alias_pairs;
    P.frames_per_wave = sh.frames_per_wave;
    if (sh.wants_geo) {
      lrp::GeoKey key;
      std::memset(&key, 0, sizeof(key));
      key.device = device;
      key.out_type = ol;
      key.in_mode = im;
      key.out_w = out->width, key.out_h = out->height, key.in_w = in->width, key.in_h = in->height;
      key.has_rot = P.has_rot;
      key.num_samples = num_samples;
      key.out_lens = lrp::geo_canonical_lens(P.out_lens, out->lens.type), key.in_lens = lrp::geo_canonical_lens(P.in_lens, in->lens.type);
      if (P.has_rot) std::memcpy(key.rot, P.rot, sizeof(key.rot));
      lrp::geo_acquire(key, sh.geo_want_boxes, stream, &geo);
      lrp::GeoFacts facts;
      facts.mode = geo.mode, facts.lists = geo.lists;
      facts.n_work = geo.n_work, facts.n_runs = geo.n_runs, facts.n_corner_blocks = geo.n_corner_blocks, facts.n_blocks = geo.n_blocks;
      facts.n_wide = geo.n_wide, facts.n_inview = geo.n_inview;
      const lrp::PlanGeo pg = lrp::plan_geo(req, sw, sh, facts);
      if (pg.geo_mode != 0) {
        P.geo_mode = pg.geo_mode;
        P.geo_xy = geo.xy;
        P.geo_box = geo.box;
        P.win_mode = pg.win_mode;
        P.quad = pg.quad;
        P.blocks_per_wave = pg.blocks_per_wave;
        P.rgbaz_runs = pg.rgbaz_runs;
        P.big_windows = pg.big_windows;
        if (pg.listed) { // rendering by block class: the lists of the entry (lrp_params.h "Block lists")
          const uint8_t *const lists = reinterpret_cast<const uint8_t *>(geo.box) + lrp::geo_lists_offset(out->width, out->height);
          P.geo_work = reinterpret_cast<const int32_t *>(lists + (size_t)lrp::kGeoListHeaderWords * 4);
          P.geo_runs = reinterpret_cast<const uint32_t *>(P.geo_work + 2 * lrp::geo_work_capacity(out->width, out->height));
          P.geo_n_work = geo.n_work;
          P.geo_n_runs = geo.n_runs;
          P.geo_work_rec = pg.list_recs ? reinterpret_cast<const int32_t *>(lists + lrp::geo_work_recs_offset(out->width, out->height)) : nullptr;
          P.geo_fill_stride = pg.fill_stride;
          P.geo_fill_per_wave = pg.fill_per_wave;
        }
      }
    }
    const bool listed = P.geo_work != nullptr;
    auto launch = [&]() {
      if (listed) { // the corner runs of this launch's frames, then (or meanwhile, or inside it) everything else
        g_knobs[kKnobListedLaunches].fetch_add(1, std::memory_order_relaxed);
        if (P.geo_fill_per_wave == 0) {
          const hipError_t fe = fill_corner_runs(P, device, stream);
          if (fe != hipSuccess) return fe;
        }
      }
      if (window && P.geo_mode == 2 && P.big_windows != 0) g_knobs[kKnobBigLaunches].fetch_add(1, std::memory_order_relaxed);
      if (window) return lrp::launch_win_bicubic(P, ol, im, stream);
      if (P.geo_mode == 2 && num_samples > 1) return lrp::launch_ss_gather(P, interpolation, im, stream); // (a lane per sub-sample: coalesced loads of the entry)
      if (interpolation == LRP_NEAREST) return lrp::launch_tile_nearest(P, ol, im, stream);
      if (interpolation == LRP_BILINEAR) return lrp::launch_tile_bilinear(P, ol, im, stream);
      return lrp::launch_tile_bicubic(P, ol, im, stream);
    };
    if (n_batch <= 0) {
      e = launch();
    } else {
      e = hipSuccess;
      int first = 0;
      if (P.geo_mode == 1 || P.geo_mode == 3) {
        // the frame that writes the entry goes alone (the instantiations without the frame loop have the side output); the
        // rest of the batch follows on the same stream and reads it
        P.src = in[0].data;
        P.dst = out[0].data;
        e = launch();
        P.geo_mode = 2;
        first = 1;
      }
      for (; first < n_batch && e == hipSuccess; first += lrp::kMaxBatch) {
        P.batch_n = std::min(lrp::kMaxBatch, n_batch - first);
        for (int i = 0; i < P.batch_n; ++i) {
          P.batch_src[i] = in[first + i].data;
          P.batch_dst[i] = out[first + i].data;
        }
        e = launch();
      }
    }
    if (e == hipSuccess && window && (geo.mode == 1 || geo.mode == 3) && geo.host_counts != nullptr) {
      // the launch above wrote the box records and the class bytes of the entry: the block lists (rectilinear source) and the
      // census of its windows are built behind it, and their header follows the records to the host (page-locked; read once
      // the records' event has completed)
      const uint8_t *const header = reinterpret_cast<const uint8_t *>(geo.box) + lrp::geo_lists_offset(out->width, out->height);
      const bool with_lists = im == lrp::kInRect && knob(kKnobGeoLists) != 0, with_census = knob(kKnobGeoCensus) != 0 && !lrp::radial_in(im);
      if (!with_lists && !with_census) {
        // (nothing to tell the host about this entry)
      } else if ((!with_lists || lrp::launch_geo_build_lists(geo.box, out->width, out->height, P.alias_pairs, stream) == hipSuccess) &&
          (!with_census || lrp::launch_geo_census(geo.box, out->width, out->height, in->width, in->height, !with_lists, stream) == hipSuccess) &&
          hipMemcpyAsync(geo.host_counts, header, (size_t)lrp::kGeoListHeaderWords * 4, hipMemcpyDeviceToHost, stream) == hipSuccess)
        geo.lists_enqueued = true;
      else
        (void)hipGetLastError(); // (no lists for this entry: every launch enumerates the frame)
    }
    lrp::geo_launched(&geo, stream, e == hipSuccess);
  } else {
    const int n = n_batch > 0 ? n_batch : 1;
    e = hipSuccess;
    // The run-time channel path holds up to 8 channels of a pixel in registers; wider texels (the
    // reference loop is generic in C, src/reproject.cpp:50,76,134) are rendered 8 channels per launch.
    // post_process touches channels 0-2 only (:423-434): they are all in the first group.
    const int C = out->channels, group = C == 4 ? 4 : 8;
    for (int i = 0; i < n && e == hipSuccess; ++i)
      for (int c0 = 0; c0 < C && e == hipSuccess; c0 += group) {
        P.src = in[i].data + c0;
        P.dst = out[i].data + c0;
        P.ch_count = std::min(group, C - c0);
        P.has_post = post != nullptr && c0 == 0;
        if (interpolation == LRP_NEAREST)
          e = lrp::launch_nearest(P, ol, im, stream);
        else if (interpolation == LRP_BILINEAR)
          e = lrp::launch_bilinear(P, ol, im, stream);
        else
          e = lrp::launch_bicubic(P, ol, im, stream);
      }
  }
  if (e != hipSuccess) return hip_fail(e, "reproject kernel launch");
  return LRP_OK;
}

// lrp_coverage_device's checks: the lens, extension and size checks of validate() in its order, then the request itself.
int validate_coverage(const lrp_image *in, const lrp_image *out, int num_samples, bool want_plane, int mask_image, int alpha_channel) {
  if (!in || !out) return fail(LRP_ERR_NULL, "null image");
  const int ext = g_lens_ext.load(std::memory_order_relaxed);
  if (!lens_in_hot_path(out->lens.type, ext)) return fail(LRP_ERR_OUTPUT_LENS, "Output lens type not supported.");
  if (!lens_in_hot_path(in->lens.type, ext)) return fail(LRP_ERR_INPUT_LENS, "Input lens type not supported.");
  if (in->width < 1 || in->height < 1 || out->width < 1 || out->height < 1)
    return fail(LRP_ERR_BAD_DIMS, "image dimensions must be positive");
  const bool touches_image = mask_image != 0 || alpha_channel != -1;
  if ((unsigned long long)out->width * (unsigned long long)out->height > kMaxImageFloats || (touches_image && out->channels >= 1 && !image_addressable(*out)))
    return fail(LRP_ERR_BAD_DIMS, "an image of more than 2^31 floats (8 GiB) cannot be addressed (the reference indexes texels with int, src/reproject.cpp:49-51)");
  if (!want_plane && !touches_image) return fail(LRP_ERR_BAD_ARG, "nothing requested: no coverage plane, no mask, no alpha channel");
  if (num_samples < 1 || num_samples > 15) return fail(LRP_ERR_BAD_ARG, "num_samples of a coverage call must be 1 .. 15 (the count is one byte)");
  if (touches_image && out->channels < 1) return fail(LRP_ERR_CHANNELS, "out->channels must be >= 1");
  if (alpha_channel < -1 || (alpha_channel >= 0 && alpha_channel >= out->channels)) return fail(LRP_ERR_BAD_ARG, "alpha_channel outside [-1, out->channels)");
  if (touches_image && !out->data) return fail(LRP_ERR_NULL, "null image data");
  return LRP_OK;
}

// One launch of the coverage kernel (lrp_coverage.hip); no table, no geometry-cache entry, no allocation.
int enqueue_coverage(const lrp_image *in, const lrp_image *out, int num_samples, const float *rotation, uint8_t *plane, int mask_image,
                     int alpha_channel, hipStream_t stream) {
  if (!lrp::launch_coverage) return fail(LRP_ERR_HIP, "the coverage kernels (lrp_coverage.hip) are not part of this build");
  const lrp::KParams P = make_params(in, out, num_samples, rotation, nullptr);
  const hipError_t e = lrp::launch_coverage(P, out->lens.type, in_lens_mode(in->lens), plane, mask_image, alpha_channel, stream);
  if (e != hipSuccess) return hip_fail(e, "coverage kernel launch");
  return LRP_OK;
}

const char *in_mode_name(int mode) {
  switch (mode) {
  case lrp::kInRect: return "rectilinear";
  case lrp::kInEquidistant: return "equidistant";
  case lrp::kInEquirect: return "clamped equirectangular";
  case lrp::kInEquirectLoop: return "wrapping equirectangular";
  case lrp::kInEquisolid: return "equisolid";
  default: return "stereographic";
  }
}

// The checks that several compose and camera entry points run, each stated once; where and in which order
// an entry point runs them is its validator's business (include/lrp.h states the order).
// Item 1 of every compose call: n_in, then mode.
int check_sources_and_mode(int n_in, int mode) {
  if (n_in < 1 || n_in > LRP_COMPOSE_MAX_SOURCES)
    return fail(LRP_ERR_BAD_ARG, "n_in of a compose call must be 1 .. " + std::to_string(LRP_COMPOSE_MAX_SOURCES));
  if (mode != LRP_COMPOSE_FIRST && mode != LRP_COMPOSE_MEAN && mode != LRP_COMPOSE_FEATHER) return fail(LRP_ERR_BAD_ARG, "unknown compose mode");
  return LRP_OK;
}

int check_compose_samples(int num_samples) {
  if (num_samples < 1 || num_samples > lrp::kComposeSsMaxSamples)
    return fail(LRP_ERR_BAD_ARG, "num_samples of a compose call must be 1 .. " + std::to_string(lrp::kComposeSsMaxSamples));
  return LRP_OK;
}

// The sampler of a camera call: the reference's three (validate() knows LRP_LANCZOS3 besides).
int check_three_samplers(int interpolation) {
  if (interpolation != LRP_NEAREST && interpolation != LRP_BILINEAR && interpolation != LRP_BICUBIC)
    return fail(LRP_ERR_INTERPOLATION, "Interpolation method not supported.");
  return LRP_OK;
}

// gains: n_in values (not null).
int check_gains(const float *gains, int n_in) {
  for (int i = 0; i < n_in; ++i)
    if (!std::isfinite(gains[i]) || gains[i] < 0.0f)
      return fail(LRP_ERR_BAD_ARG, "camera " + std::to_string(i) + ": gain must be finite and not negative");
  return LRP_OK;
}

// What an overlap call checks behind its cameras and its output.
int check_overlap(const uint64_t *stats, float lo, float hi) {
  if (!stats) return fail(LRP_ERR_NULL, "null stats");
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(0.0f <= lo && lo <= hi && hi <= 32768.0f))
    return fail(LRP_ERR_BAD_ARG, "lo and hi of an overlap call must be finite with 0 <= lo <= hi <= 32768");
  return LRP_OK;
}

// lrp_compose_device's checks, in the order include/lrp.h states.
int validate_compose(const lrp_image *ins, int n_in, const lrp_image *out, int interpolation, int mode) {
  int st = check_sources_and_mode(n_in, mode);
  if (st != LRP_OK) return st;
  if (!ins || !out) return fail(LRP_ERR_NULL, "null image");
  for (int i = 0; i < n_in; ++i) { // (in->channels == out->channels is one of validate()'s checks)
    st = validate(ins + i, out, interpolation, true, false);
    if (st != LRP_OK) return st;
  }
  const int first = in_lens_mode(ins[0].lens);
  for (int i = 1; i < n_in; ++i)
    if (in_lens_mode(ins[i].lens) != first)
      return fail(LRP_ERR_BAD_ARG, std::string("the sources of a compose call must be of one source mode: source 0 is ") + in_mode_name(first) + ", source " +
                                       std::to_string(i) + " is " + in_mode_name(in_lens_mode(ins[i].lens)));
  return LRP_OK;
}

// The ideal-lens sources of a compose block (ComposeParams, ComposeSsParams, ComposePackedParams; the block must be zeroed): per
// source the values make_params() packs for a reprojection of source i — none of those taken depends on num_samples — and its data
// pointer; the output's size, lens and tonemap from source 0; n_src and mode.
template <class Block>
void pack_ideal_sources(Block &C, const lrp_image *ins, int n_in, const float *rotations, const lrp_image *out, int mode, const lrp_post *post) {
  for (int i = 0; i < n_in; ++i) {
    const lrp::KParams P = make_params(ins + i, out, 1, rotations ? rotations + 9 * i : nullptr, post);
    if (i == 0) {
      C.out_w = P.out_w, C.out_h = P.out_h, C.channels = P.channels;
      C.out_lens = P.out_lens;
      C.has_post = P.has_post;
      C.exposure = P.exposure, C.reinhard = P.reinhard;
    }
    auto &S = C.src[i];
    S.data = ins[i].data;
    S.in_w = P.in_w, S.in_h = P.in_h;
    S.lens = P.in_lens;
    S.has_rot = P.has_rot;
    std::memcpy(S.rot, P.rot, sizeof(S.rot));
  }
  C.n_src = n_in;
  C.mode = mode;
}

// One launch per group of 8 channels of a float32 compose block whose sources (src[i].data: channel 0 of source i) and n_src are
// packed: the loop moves the sources' pointers and dst to the group's first channel and states ch_count and has_post, launch(c0)
// enqueues the block as it then stands.  `what` names the launch in lrp_last_error.
template <class Block, class Launch>
int launch_channel_groups(Block &C, float *dst, int channels, const lrp_post *post, const char *what, Launch launch) {
  const float *base[lrp::kComposeMaxSources];
  for (int i = 0; i < C.n_src; ++i) base[i] = C.src[i].data;
  const int group = lrp::kComposeMaxChannels;
  for (int c0 = 0; c0 < channels; c0 += group) {
    for (int i = 0; i < C.n_src; ++i) C.src[i].data = base[i] + c0;
    C.dst = dst + c0;
    C.ch_count = std::min(group, channels - c0);
    C.has_post = post != nullptr && c0 == 0; // (the tonemap touches channels 0-2)
    const hipError_t e = launch(c0);
    if (e != hipSuccess) return hip_fail(e, what);
  }
  return LRP_OK;
}

// One launch of the compose kernel per group of 8 channels (lrp_compose.hip); no table, no geometry-cache entry, no allocation.
int enqueue_compose(const lrp_image *ins, int n_in, const float *rotations, const lrp_image *out, int interpolation, int mode,
                    const lrp_post *post, uint8_t *count, hipStream_t stream) {
  if (!lrp::launch_compose) return fail(LRP_ERR_HIP, "the compose kernels (lrp_compose.hip) are not part of this build");
  lrp::ComposeParams C;
  std::memset(&C, 0, sizeof(C));
  pack_ideal_sources(C, ins, n_in, rotations, out, mode, post);
  return launch_channel_groups(C, out->data, out->channels, post, "compose kernel launch", [&](int c0) {
    C.count = c0 == 0 ? count : nullptr; // (k does not depend on the channels: the first group writes it)
    return lrp::launch_compose(C, out->lens.type, in_lens_mode(ins[0].lens), interpolation, stream);
  });
}

// One launch of the supersampled compose kernel per group of 8 channels (lrp_compose_ss.hip), each of which writes the planes;
// no table, no geometry-cache entry, no allocation.
int enqueue_compose_ss(const lrp_image *ins, int n_in, const float *rotations, const lrp_image *out, int num_samples, int interpolation,
                       int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage, hipStream_t stream) {
  if (!lrp::launch_compose_ss) return fail(LRP_ERR_HIP, "the supersampled compose kernels (lrp_compose_ss.hip) are not part of this build");
  lrp::ComposeSsParams C;
  std::memset(&C, 0, sizeof(C));
  pack_ideal_sources(C, ins, n_in, rotations, out, mode, post);
  C.num_samples = num_samples;
  C.count = count;
  C.coverage = coverage;
  return launch_channel_groups(C, out->data, out->channels, post, "supersampled compose kernel launch", [&](int) {
    return lrp::launch_compose_ss(C, out->lens.type, in_lens_mode(ins[0].lens), interpolation, stream);
  });
}

static_assert((int)lrp::kCameraBrown == LRP_CAMERA_BROWN && (int)lrp::kCameraFisheye == LRP_CAMERA_FISHEYE, "lrp_camera.h numbers camera models like include/lrp.h");

// The coefficients of a camera's radial polynomial x * (1 + c[0] x^2 + c[1] x^4 + c[2] x^6 + c[3] x^8): x is r (BROWN: k1 k2 k3) or
// theta (FISHEYE: k1 .. k4).  Returns how many of cam->k the model uses.
int camera_radial(const lrp_camera &cam, double c[4]) {
  if (cam.model == LRP_CAMERA_FISHEYE) {
    for (int j = 0; j < 4; ++j) c[j] = cam.k[j];
    return 4;
  }
  c[0] = cam.k[0], c[1] = cam.k[1], c[2] = cam.k[4], c[3] = 0.0;
  return 5;
}

// The checks of one camera, in the order include/lrp.h states: model, size (with `channels`), data (a source; a target's is
// ignored), intrinsics, the used coefficients, limit.  `who` starts the lrp_last_error text.
int validate_camera(const lrp_camera &cam, const std::string &who, int channels, bool needs_data) {
  if (cam.model != LRP_CAMERA_BROWN && cam.model != LRP_CAMERA_FISHEYE) return fail(LRP_ERR_BAD_ARG, who + "unknown model");
  if (cam.width < 1 || cam.height < 1) return fail(LRP_ERR_BAD_DIMS, who + "width and height must be positive");
  if ((unsigned long long)cam.width * (unsigned long long)cam.height * (unsigned long long)channels > kMaxImageFloats)
    return fail(LRP_ERR_BAD_DIMS, who + "a frame of more than 2^31 floats (8 GiB) cannot be addressed");
  if (needs_data && !cam.data) return fail(LRP_ERR_NULL, who + "data is null");
  const float intrinsics[4] = {cam.fx, cam.fy, cam.cx, cam.cy};
  static const char *const names[4] = {"fx", "fy", "cx", "cy"};
  for (int j = 0; j < 4; ++j)
    if (!std::isfinite(intrinsics[j])) return fail(LRP_ERR_BAD_ARG, who + names[j] + " is not finite");
  double c[4];
  const int used = camera_radial(cam, c);
  for (int j = 0; j < used; ++j)
    if (!std::isfinite(cam.k[j])) return fail(LRP_ERR_BAD_ARG, who + "k[" + std::to_string(j) + "] is not finite");
  if (cam.fx == 0.0f) return fail(LRP_ERR_BAD_ARG, who + "fx must not be 0");
  if (cam.fy == 0.0f) return fail(LRP_ERR_BAD_ARG, who + "fy must not be 0");
  if (!(cam.limit >= 0.0f)) return fail(LRP_ERR_BAD_ARG, who + "limit must be >= 0 (+inf allowed)");
  return LRP_OK;
}

// Items 1 to 5 of lrp_compose_cameras_device's checks, in the order include/lrp.h states.  gains: checked for NULL with item 2
// when wants_gains (lrp_compose_cameras_gain_device); needs_out_data: false for a call that writes no image
// (lrp_camera_overlap_device).
int validate_cameras_and_output(const lrp_camera *cams, int n_in, const lrp_image *out, int interpolation, int mode, bool needs_out_data,
                                bool wants_gains, const float *gains) {
  int st = check_sources_and_mode(n_in, mode);
  if (st != LRP_OK) return st;
  if (!cams || !out) return fail(LRP_ERR_NULL, cams ? "null image" : "null camera array");
  if (wants_gains && !gains) return fail(LRP_ERR_NULL, "null gains");
  if (!lens_in_hot_path(out->lens.type, g_lens_ext.load(std::memory_order_relaxed))) return fail(LRP_ERR_OUTPUT_LENS, "Output lens type not supported.");
  if (out->channels < 1) return fail(LRP_ERR_CHANNELS, "out->channels must be >= 1");
  if (out->width < 1 || out->height < 1) return fail(LRP_ERR_BAD_DIMS, "image dimensions must be positive");
  if (!image_addressable(*out)) return fail(LRP_ERR_BAD_DIMS, "an image of more than 2^31 floats (8 GiB) cannot be addressed");
  if (needs_out_data && !out->data) return fail(LRP_ERR_NULL, "null image data");
  st = check_three_samplers(interpolation);
  if (st != LRP_OK) return st;
  for (int i = 0; i < n_in; ++i) {
    st = validate_camera(cams[i], "camera " + std::to_string(i) + ": ", out->channels, true);
    if (st != LRP_OK) return st;
  }
  return LRP_OK;
}

// lrp_compose_cameras_device's checks, in the order include/lrp.h states.
int validate_compose_cameras(const lrp_camera *cams, int n_in, const lrp_image *out, int num_samples, int interpolation, int mode) {
  const int st = validate_cameras_and_output(cams, n_in, out, interpolation, mode, true, false, nullptr);
  if (st != LRP_OK) return st;
  return check_compose_samples(num_samples);
}

// What the kernels read of a camera besides its data pointer and its rotation.
void pack_camera(lrp::CameraSource &S, const lrp_camera &cam) {
  S.in_w = cam.width, S.in_h = cam.height;
  S.model = cam.model;
  S.fx = cam.fx, S.fy = cam.fy, S.cx = cam.cx, S.cy = cam.cy;
  std::memcpy(S.k, cam.k, sizeof(S.k));
  S.limit = cam.limit;
}

// The camera descriptors of a block (zeroed), whole: pack_camera, the data pointer — channel 0; launch_channel_groups moves it —
// and camera i's rotation, rotations + 9 * i.
void pack_cameras(lrp::CameraSource src[], const lrp_camera *cams, int n_in, const float *rotations) {
  for (int i = 0; i < n_in; ++i) {
    lrp::CameraSource &S = src[i];
    pack_camera(S, cams[i]);
    S.data = cams[i].data;
    S.has_rot = rotations != nullptr;
    if (rotations) std::memcpy(S.rot, rotations + 9 * i, sizeof(S.rot));
  }
}

// The fields the camera compose blocks share besides their descriptors (CameraParams, CameraGainParams::cam, CameraViewParams,
// CameraPackedParams; the block must be zeroed): the output's size, the tonemap's constants, n_src, mode, num_samples and the planes.
template <class Block>
void set_camera_fields(Block &C, int out_w, int out_h, int channels, int n_in, int mode, int num_samples, const lrp_post *post, uint8_t *count,
                       uint8_t *coverage) {
  C.out_w = out_w, C.out_h = out_h, C.channels = channels;
  if (post) C.exposure = post->exposure, C.reinhard = post->reinhard;
  C.n_src = n_in;
  C.mode = mode;
  C.num_samples = num_samples;
  C.count = count;
  C.coverage = coverage;
}

// One launch of the camera compose kernel per group of 8 channels (lrp_camera.hip), each of which writes the planes; no table, no
// geometry-cache entry, no allocation.
int enqueue_compose_cameras(const lrp_camera *cams, int n_in, const float *rotations, const lrp_image *out, int num_samples, int interpolation,
                            int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage, hipStream_t stream) {
  if (!lrp::launch_compose_cameras) return fail(LRP_ERR_HIP, "the camera compose kernels (lrp_camera.hip) are not part of this build");
  lrp::CameraParams C;
  std::memset(&C, 0, sizeof(C));
  set_camera_fields(C, out->width, out->height, out->channels, n_in, mode, num_samples, post, count, coverage);
  C.out_lens = pack_lens(out->lens);
  pack_cameras(C.src, cams, n_in, rotations);
  return launch_channel_groups(C, out->data, out->channels, post, "camera compose kernel launch",
                               [&](int) { return lrp::launch_compose_cameras(C, out->lens.type, interpolation, stream); });
}

static_assert(lrp::kOverlapWords == LRP_OVERLAP_WORDS, "lrp_camstat.h states the table size of include/lrp.h");

// The launcher (lrp_camstat.hip) zeroes the table on `stream` ahead of the one launch of the overlap kernel, which adds into it; no
// allocation, no synchronisation, no geometry-cache entry.
int enqueue_camera_overlap(const lrp_camera *cams, int n_in, const float *rotations, const lrp_image *out, float lo, float hi, uint64_t *stats,
                           hipStream_t stream) {
  if (!lrp::launch_camera_overlap) return fail(LRP_ERR_HIP, "the camera overlap kernels (lrp_camstat.hip) are not part of this build");
  lrp::CameraStatParams C;
  std::memset(&C, 0, sizeof(C));
  C.stats = reinterpret_cast<unsigned long long *>(stats);
  C.out_w = out->width, C.out_h = out->height, C.channels = out->channels;
  C.ch_count = std::min(out->channels, 3);
  C.out_lens = pack_lens(out->lens);
  C.n_src = n_in;
  C.lo = lo, C.hi = hi;
  pack_cameras(C.src, cams, n_in, rotations);
  const hipError_t e = lrp::launch_camera_overlap(C, out->lens.type, stream);
  if (e != hipSuccess) return hip_fail(e, "zeroing the overlap table or the camera overlap kernel launch");
  return LRP_OK;
}

// enqueue_compose_cameras with gains: the first group of 8 channels — the one that holds the colour channels — goes through the
// gain kernel (lrp_camgain.hip), the further groups, which the gains do not touch, through the camera compose kernel itself.
int enqueue_compose_cameras_gain(const lrp_camera *cams, int n_in, const float *rotations, const float *gains, const lrp_image *out,
                                 int num_samples, int interpolation, int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage,
                                 hipStream_t stream) {
  if (!lrp::launch_compose_cameras_gain) return fail(LRP_ERR_HIP, "the camera gain compose kernels (lrp_camgain.hip) are not part of this build");
  if (!lrp::launch_compose_cameras) return fail(LRP_ERR_HIP, "the camera compose kernels (lrp_camera.hip) are not part of this build");
  lrp::CameraGainParams G;
  std::memset(&G, 0, sizeof(G));
  lrp::CameraParams &C = G.cam;
  set_camera_fields(C, out->width, out->height, out->channels, n_in, mode, num_samples, post, count, coverage);
  C.out_lens = pack_lens(out->lens);
  pack_cameras(C.src, cams, n_in, rotations);
  for (int i = 0; i < n_in; ++i) G.gain[i] = gains[i];
  return launch_channel_groups(C, out->data, out->channels, post, "camera gain compose kernel launch", [&](int c0) {
    return c0 == 0 ? lrp::launch_compose_cameras_gain(G, out->lens.type, interpolation, stream)
                   : lrp::launch_compose_cameras(C, out->lens.type, interpolation, stream);
  });
}

static_assert(lrp::kCameraInverseSteps == LRP_CAMERA_INVERSE_STEPS, "lrp_camera_inverse.h takes the step count of include/lrp.h");

// lrp_camera_view_device's checks, in the order include/lrp.h states.
int validate_camera_view(const lrp_camera *cams, int n_in, const lrp_camera *target, const float *out_data, int channels, int num_samples,
                         int interpolation, int mode) {
  int st = check_sources_and_mode(n_in, mode);
  if (st != LRP_OK) return st;
  if (!cams || !target || !out_data) return fail(LRP_ERR_NULL, !cams ? "null camera array" : !target ? "null target camera" : "null output data");
  st = validate_camera(*target, "target: ", std::max(channels, 1), false); // (channels < 1 is the next check's)
  if (st != LRP_OK) return st;
  if (channels < 1) return fail(LRP_ERR_CHANNELS, "channels must be >= 1");
  st = check_three_samplers(interpolation);
  if (st != LRP_OK) return st;
  for (int i = 0; i < n_in; ++i) {
    st = validate_camera(cams[i], "camera " + std::to_string(i) + ": ", channels, true);
    if (st != LRP_OK) return st;
  }
  return check_compose_samples(num_samples);
}

// One launch of the camera-view kernel per group of 8 channels (lrp_camview.hip), each of which writes the planes; no table, no
// geometry-cache entry, no allocation.
int enqueue_camera_view(const lrp_camera *cams, int n_in, const float *rotations, const lrp_camera *target, float *out_data, int channels,
                        int num_samples, int interpolation, int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage, hipStream_t stream) {
  if (!lrp::launch_camera_view) return fail(LRP_ERR_HIP, "the camera-view kernels (lrp_camview.hip) are not part of this build");
  lrp::CameraViewParams C;
  std::memset(&C, 0, sizeof(C));
  set_camera_fields(C, target->width, target->height, channels, n_in, mode, num_samples, post, count, coverage);
  pack_camera(C.target, *target);
  pack_cameras(C.src, cams, n_in, rotations);
  return launch_channel_groups(C, out_data, channels, post, "camera-view kernel launch",
                               [&](int) { return lrp::launch_camera_view(C, interpolation, stream); });
}

static_assert((int)lrp::kPackedF32 == LRP_PIXEL_F32 && (int)lrp::kPackedF16 == LRP_PIXEL_F16 && (int)lrp::kPackedU8 == LRP_PIXEL_U8_GAMMA, "lrp_packed.h numbers pixel formats like include/lrp.h");

bool format_ok(int f) { return f == LRP_PIXEL_F32 || f == LRP_PIXEL_F16 || f == LRP_PIXEL_U8_GAMMA; }

// The packed image of `packed_channels` samples per pixel fits the byte offsets of the packed kernel (32-bit): the size limit of
// validate() — 2^31 — applied to bytes.  (Dimensions are positive: validate() ran.)
bool packed_addressable(const lrp_image &im, int format, int packed_channels) {
  const unsigned long long px = (unsigned long long)im.width * (unsigned long long)im.height; // < 2^62
  const unsigned long long sample = lrp::pixel_bytes(format, 1);
  return px <= kMaxImageFloats / sample && (unsigned long long)packed_channels <= kMaxImageFloats / (px * sample);
}

// What every packed call adds to the checks of its float32 parent ahead of the sizes in bytes, in the order include/lrp.h states:
// a float32 source (`float32_needs`: the subject and verb of the call's text, `instead`: the calls it names), the formats (has_out
// false: a call without a packed output), the packed channel counts, C (`who_does`: the entry point and its verb, in front of "at
// most 4 channels").
int check_packed_formats(int in_format, int in_pch, bool has_out, int out_format, int out_pch, int channels, const char *float32_needs,
                         const char *instead, const char *who_does) {
  if (in_format == LRP_PIXEL_F32) return fail(LRP_ERR_BAD_ARG, std::string(float32_needs) + " no decode: call " + instead);
  if (!format_ok(in_format) || (has_out && !format_ok(out_format))) return fail(LRP_ERR_BAD_ARG, "unknown pixel format");
  if (in_pch < 1 || (has_out && out_pch < 1)) return fail(LRP_ERR_BAD_ARG, "packed channel counts must be >= 1");
  if (channels > lrp::kPackedMaxChannels)
    return fail(LRP_ERR_CHANNELS, std::string(who_does) + " at most " + std::to_string(lrp::kPackedMaxChannels) + " channels");
  return LRP_OK;
}

// lrp_reproject_packed_device's checks, in the order include/lrp.h states.
int validate_packed(const lrp_image *in, int in_format, int in_pch, const lrp_image *out, int out_format, int out_pch, int interpolation) {
  int st = validate(in, out, interpolation, true, false);
  if (st != LRP_OK) return st;
  st = check_packed_formats(in_format, in_pch, true, out_format, out_pch, in->channels, "a float32 source needs",
                            "lrp_reproject_device + lrp_encode_pixels_device", "lrp_reproject_packed_device renders");
  if (st != LRP_OK) return st;
  if (!packed_addressable(*in, in_format, in_pch) || !packed_addressable(*out, out_format, out_pch))
    return fail(LRP_ERR_BAD_DIMS, "a packed image of more than 2^31 bytes cannot be addressed (the packed kernel forms 32-bit byte offsets)");
  return LRP_OK;
}

// One launch of the packed kernel (lrp_packed.hip).  num_samples == 1: through the geometry cache, under the key
// enqueue_reproject builds for this geometry — the entry is shared with lrp_reproject_device in both directions.
int enqueue_packed(const lrp_image *in, int in_format, int in_pch, lrp_image *out, int out_format, int out_pch, unsigned out_fill,
                   int num_samples, int interpolation, const float *rotation, const lrp_post *post, int device, hipStream_t stream) {
  if (num_samples <= 0) return LRP_OK; // reference loop body never runs: output untouched
  if (!lrp::launch_packed) return fail(LRP_ERR_HIP, "the packed-pixel kernels (lrp_packed.hip) are not part of this build");
  const lrp::KParams K = make_params(in, out, num_samples, rotation, post);
  lrp::PackedParams P;
  std::memset(&P, 0, sizeof(P));
  P.src = in->data, P.dst = out->data;
  P.in_w = K.in_w, P.in_h = K.in_h, P.out_w = K.out_w, P.out_h = K.out_h;
  P.channels = K.channels;
  P.in_channels = in_pch, P.out_channels = out_pch;
  P.out_format = out_format;
  P.out_fill = out_fill;
  P.num_samples = K.num_samples;
  P.normalize = K.normalize;
  P.in_lens = K.in_lens, P.out_lens = K.out_lens;
  std::memcpy(P.rot, K.rot, sizeof(P.rot));
  P.has_rot = K.has_rot, P.has_post = K.has_post;
  P.exposure = K.exposure, P.reinhard = K.reinhard;
  const int ol = out->lens.type, im = in_lens_mode(in->lens);
  lrp::GeoUse geo;
  if (num_samples == 1 && knob(kKnobGeoCache) != 0) {
    lrp::GeoKey key;
    std::memset(&key, 0, sizeof(key));
    key.device = device;
    key.out_type = ol;
    key.in_mode = im;
    key.out_w = out->width, key.out_h = out->height, key.in_w = in->width, key.in_h = in->height;
    key.has_rot = P.has_rot;
    key.num_samples = num_samples;
    key.out_lens = lrp::geo_canonical_lens(P.out_lens, out->lens.type), key.in_lens = lrp::geo_canonical_lens(P.in_lens, in->lens.type);
    if (P.has_rot) std::memcpy(key.rot, P.rot, sizeof(key.rot));
    lrp::geo_acquire(key, /*want_boxes=*/false, stream, &geo);
    if (geo.mode == 1 || geo.mode == 2) {
      P.geo_mode = geo.mode;
      P.geo_xy = geo.xy;
    }
  }
  const hipError_t e = lrp::launch_packed(P, in_format, ol, im, interpolation, device, stream);
  lrp::geo_launched(&geo, stream, e == hipSuccess);
  if (e != hipSuccess) return hip_fail(e, "packed-pixel kernel launch");
  return LRP_OK;
}

// lrp_compose_packed_device's checks, in the order include/lrp.h states: those of lrp_compose_device, then those
// lrp_reproject_packed_device adds to lrp_reproject_device's.
int validate_compose_packed(const lrp_image *ins, int n_in, int in_format, int in_pch, const lrp_image *out, int out_format, int out_pch,
                            int interpolation, int mode) {
  int st = validate_compose(ins, n_in, out, interpolation, mode);
  if (st != LRP_OK) return st;
  st = check_packed_formats(in_format, in_pch, true, out_format, out_pch, out->channels, "float32 sources need",
                            "lrp_compose_device + lrp_encode_pixels_device", "lrp_compose_packed_device composes");
  if (st != LRP_OK) return st;
  bool fits = packed_addressable(*out, out_format, out_pch);
  for (int i = 0; i < n_in; ++i) fits = fits && packed_addressable(ins[i], in_format, in_pch);
  if (!fits) return fail(LRP_ERR_BAD_DIMS, "a packed image of more than 2^31 bytes cannot be addressed (the packed compose kernel forms 32-bit byte offsets)");
  return LRP_OK;
}

// One launch of the packed compose kernel (lrp_compose_packed.hip); no table but the two 8-bit ones, no geometry-cache entry, no
// allocation.
int enqueue_compose_packed(const lrp_image *ins, int n_in, int in_format, int in_pch, const float *rotations, const lrp_image *out,
                           int out_format, int out_pch, unsigned out_fill, int interpolation, int mode, const lrp_post *post, uint8_t *count,
                           int device, hipStream_t stream) {
  if (!lrp::launch_compose_packed) return fail(LRP_ERR_HIP, "the packed compose kernels (lrp_compose_packed.hip) are not part of this build");
  lrp::ComposePackedParams C;
  std::memset(&C, 0, sizeof(C));
  pack_ideal_sources(C, ins, n_in, rotations, out, mode, post);
  C.dst = out->data;
  C.count = count;
  C.in_channels = in_pch, C.out_channels = out_pch;
  C.out_format = out_format;
  C.out_fill = out_fill;
  const hipError_t e = lrp::launch_compose_packed(C, in_format, out->lens.type, in_lens_mode(ins[0].lens), interpolation, device, stream);
  if (e != hipSuccess) return hip_fail(e, "packed compose kernel launch");
  return LRP_OK;
}

// What the packed camera calls add to the checks of their float32 parents, in the order include/lrp.h states:
// check_packed_formats (who_takes: the entry point and "takes", instead: the calls for float32 frames), then the sizes in bytes.
// (Dimensions are positive: the parents' checks ran.)
int validate_cameras_packed(const lrp_camera *cams, int n_in, int in_format, int in_pch, const lrp_image *out, bool has_out, int out_format,
                            int out_pch, const char *who_takes, const char *instead) {
  const int st = check_packed_formats(in_format, in_pch, has_out, out_format, out_pch, out->channels, "float32 frames need", instead, who_takes);
  if (st != LRP_OK) return st;
  bool fits = !has_out || packed_addressable(*out, out_format, out_pch);
  for (int i = 0; i < n_in; ++i) {
    lrp_image frame;
    std::memset(&frame, 0, sizeof(frame));
    frame.width = cams[i].width, frame.height = cams[i].height;
    fits = fits && packed_addressable(frame, in_format, in_pch);
  }
  if (!fits) return fail(LRP_ERR_BAD_DIMS, "a packed frame or output of more than 2^31 bytes cannot be addressed (the packed camera kernels form 32-bit byte offsets)");
  return LRP_OK;
}

// One launch of the packed camera compose kernel (lrp_camera_packed.hip); no table but the two 8-bit ones, no geometry-cache
// entry, no allocation.  gains == nullptr: a gain of 1.0f per camera.
int enqueue_compose_cameras_packed(const lrp_camera *cams, int n_in, int in_format, int in_pch, const float *rotations, const float *gains,
                                   const lrp_image *out, int out_format, int out_pch, unsigned out_fill, int num_samples, int interpolation,
                                   int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage, int device, hipStream_t stream) {
  if (!lrp::launch_compose_cameras_packed) return fail(LRP_ERR_HIP, "the packed camera compose kernels (lrp_camera_packed.hip) are not part of this build");
  lrp::CameraPackedParams C;
  std::memset(&C, 0, sizeof(C));
  set_camera_fields(C, out->width, out->height, out->channels, n_in, mode, num_samples, post, count, coverage);
  C.dst = out->data;
  C.in_channels = in_pch, C.out_channels = out_pch;
  C.out_format = out_format;
  C.out_fill = out_fill;
  C.out_lens = pack_lens(out->lens);
  C.has_post = post != nullptr;
  pack_cameras(C.src, cams, n_in, rotations);
  for (int i = 0; i < n_in; ++i) C.gain[i] = gains ? gains[i] : 1.0f;
  const hipError_t e = lrp::launch_compose_cameras_packed(C, in_format, out->lens.type, interpolation, device, stream);
  if (e != hipSuccess) return hip_fail(e, "packed camera compose kernel launch");
  return LRP_OK;
}

// The launcher (lrp_camstat_packed.hip) zeroes the table on `stream` ahead of the one launch of the packed overlap kernel, which
// adds into it; no allocation, no geometry-cache entry.
int enqueue_camera_overlap_packed(const lrp_camera *cams, int n_in, int in_format, int in_pch, const float *rotations, const lrp_image *out,
                                  float lo, float hi, uint64_t *stats, int device, hipStream_t stream) {
  if (!lrp::launch_camera_overlap_packed) return fail(LRP_ERR_HIP, "the packed camera overlap kernels (lrp_camstat_packed.hip) are not part of this build");
  lrp::CameraStatPackedParams C;
  std::memset(&C, 0, sizeof(C));
  C.stats = reinterpret_cast<unsigned long long *>(stats);
  C.out_w = out->width, C.out_h = out->height, C.channels = out->channels;
  C.in_channels = in_pch;
  C.out_lens = pack_lens(out->lens);
  C.n_src = n_in;
  C.lo = lo, C.hi = hi;
  pack_cameras(C.src, cams, n_in, rotations);
  const hipError_t e = lrp::launch_camera_overlap_packed(C, in_format, out->lens.type, device, stream);
  if (e != hipSuccess) return hip_fail(e, "zeroing the overlap table or the packed camera overlap kernel launch");
  return LRP_OK;
}

static_assert(lrp::kMultibandMaxBands == LRP_MULTIBAND_MAX_BANDS && lrp::kMultibandNoCamera == LRP_MULTIBAND_NO_CAMERA, "lrp_multiband.h states the limits of include/lrp.h");

// Items 1 to 6 of lrp_compose_cameras_multiband_device, in the order include/lrp.h states; its packed twin runs them first.
int validate_multiband(const lrp_camera *cams, int n_in, const float *gains, const lrp_image *out, int interpolation, int num_bands,
                       const void *scratch, size_t scratch_bytes) {
  int st = validate_cameras_and_output(cams, n_in, out, interpolation, LRP_COMPOSE_FIRST, true, false, nullptr);
  if (st != LRP_OK) return st;
  if (gains) {
    st = check_gains(gains, n_in);
    if (st != LRP_OK) return st;
  }
  if (out->channels > lrp::kMultibandMaxChannels) return fail(LRP_ERR_CHANNELS, "out->channels of a multi-band call must be 1 .. 4");
  if (num_bands < 0 || num_bands > LRP_MULTIBAND_MAX_BANDS) return fail(LRP_ERR_BAD_ARG, "num_bands must be 0 .. " + std::to_string(LRP_MULTIBAND_MAX_BANDS));
  if (!scratch) return fail(LRP_ERR_NULL, "null scratch");
  const size_t need = lrp::multiband_layout(out->width, out->height, out->channels, num_bands).total;
  if ((reinterpret_cast<uintptr_t>(scratch) & 255u) != 0u || scratch_bytes < need)
    return fail(LRP_ERR_BAD_ARG, "scratch must be aligned to 256 bytes and hold what lrp_multiband_scratch_bytes states: scratch_bytes is " +
                                     std::to_string(scratch_bytes) + ", the call needs " + std::to_string(need));
  if (out->height > lrp::kMultibandMaxHeight)
    return fail(LRP_ERR_BAD_DIMS, "out->height of a multi-band call must be at most " + std::to_string(lrp::kMultibandMaxHeight));
  return LRP_OK;
}

// Multi-band blending (lrp_multiband*.hip), every launch on `stream`, in this order: the label kernel; then per camera its
// level-0 layer by the one-camera compose kernels (FIRST, no post, no planes) into the scratch, B reduce launches and B + 1
// Laplacian-accumulate launches; then B + 1 collapse launches from the top level down, the last of which writes the output.  No
// allocation, no synchronisation, no table, no geometry-cache entry.
// `packed` (lrp_compose_cameras_multiband_packed_device): the frames and the output are packed.  Two launches differ: a camera's
// level-0 layer is the one-camera packed compose kernel with a float32 output of C samples, and the level-0 collapse is
// lrp_mb_packed.hip's, which encodes.  Both read the device copy of the two 8-bit tables, which the first packed call on a device
// uploads; every other launch is the float call's.
struct MultibandPacked {
  int in_format, in_pch, out_format, out_pch;
  unsigned out_fill;
  int device;
};
int enqueue_multiband(const lrp_camera *cams, int n_in, const float *rotations, const float *gains, const lrp_image *out, int interpolation,
                      int num_bands, const lrp_post *post, uint8_t *count, uint8_t *label, void *scratch, const MultibandPacked *packed,
                      hipStream_t stream) {
  if (!lrp::launch_multiband_label || !lrp::launch_multiband_reduce || !lrp::launch_multiband_lap || !lrp::launch_multiband_collapse)
    return fail(LRP_ERR_HIP, "the multi-band kernels (lrp_multiband.hip, lrp_multiband_label.hip) are not part of this build");
  if (packed && !lrp::launch_mb_collapse_packed)
    return fail(LRP_ERR_HIP, "the packed multi-band collapse kernels (lrp_mb_packed.hip) are not part of this build");
  const int C = out->channels, B = num_bands;
  const lrp::MultibandLayout L = lrp::multiband_layout(out->width, out->height, C, B);
  char *const base = static_cast<char *>(scratch);
  const auto plane = [&](size_t at) { return reinterpret_cast<float *>(base + at); };
  if (!label) label = reinterpret_cast<uint8_t *>(base + L.label);
  if (!count) count = reinterpret_cast<uint8_t *>(base + L.count);
  const int wrap = out->lens.type == LRP_EQUIRECTANGULAR && source_wraps(out->lens);

  lrp::MultibandLabelParams LP;
  std::memset(&LP, 0, sizeof(LP));
  LP.label = label, LP.count = count;
  LP.out_w = out->width, LP.out_h = out->height;
  LP.n_src = n_in;
  LP.out_lens = pack_lens(out->lens);
  pack_cameras(LP.src, cams, n_in, rotations); // (the data pointers ride along: the label kernel reads the geometry only)
  hipError_t e = lrp::launch_multiband_label(LP, out->lens.type, stream);
  if (e != hipSuccess) return hip_fail(e, "multi-band label kernel launch");

  lrp_image layer = *out; // camera i's G_0: the output's lens and size, in the scratch
  layer.data = plane(L.g[0]);
  for (int i = 0; i < n_in; ++i) {
    const float *rot = rotations ? rotations + 9 * i : nullptr;
    const int st = packed ? enqueue_compose_cameras_packed(cams + i, 1, packed->in_format, packed->in_pch, rot, gains ? gains + i : nullptr, &layer,
                                                           LRP_PIXEL_F32, C, 0u, 1, interpolation, LRP_COMPOSE_FIRST, nullptr, nullptr, nullptr,
                                                           packed->device, stream)
                   : gains ? enqueue_compose_cameras_gain(cams + i, 1, rot, gains + i, &layer, 1, interpolation, LRP_COMPOSE_FIRST, nullptr, nullptr,
                                                          nullptr, stream)
                           : enqueue_compose_cameras(cams + i, 1, rot, &layer, 1, interpolation, LRP_COMPOSE_FIRST, nullptr, nullptr, nullptr, stream);
    if (st != LRP_OK) return st;
    for (int k = 0; k < B; ++k) {
      lrp::MultibandReduceParams R;
      std::memset(&R, 0, sizeof(R));
      R.g = plane(L.g[k]), R.m = k > 0 ? plane(L.m[k]) : nullptr, R.label = k > 0 ? nullptr : label;
      R.cg = plane(L.g[k + 1]), R.cm = plane(L.m[k + 1]);
      R.w = L.w[k], R.h = L.h[k], R.cw = L.w[k + 1], R.ch = L.h[k + 1];
      R.cam = i, R.wrap = wrap;
      e = lrp::launch_multiband_reduce(R, C, stream);
      if (e != hipSuccess) return hip_fail(e, "multi-band reduce kernel launch");
    }
    for (int k = 0; k <= B; ++k) {
      lrp::MultibandLapParams A;
      std::memset(&A, 0, sizeof(A));
      A.g = plane(L.g[k]), A.m = k > 0 ? plane(L.m[k]) : nullptr, A.label = k > 0 ? nullptr : label;
      A.a = plane(L.a[k]), A.s = plane(L.s[k]);
      A.w = L.w[k], A.h = L.h[k];
      A.top = k == B;
      if (!A.top) A.cg = plane(L.g[k + 1]), A.cw = L.w[k + 1], A.ch = L.h[k + 1];
      A.cam = i, A.wrap = wrap, A.first = i == 0;
      e = lrp::launch_multiband_lap(A, C, stream);
      if (e != hipSuccess) return hip_fail(e, "multi-band Laplacian-accumulate kernel launch");
    }
  }
  for (int k = B; k >= (packed ? 1 : 0); --k) {
    lrp::MultibandCollapseParams K;
    std::memset(&K, 0, sizeof(K));
    K.a = plane(L.a[k]), K.s = plane(L.s[k]);
    K.w = L.w[k], K.h = L.h[k];
    K.top = k == B;
    if (!K.top) K.cr = plane(L.a[k + 1]), K.cw = L.w[k + 1], K.ch = L.h[k + 1];
    K.wrap = wrap;
    K.dst = k == 0 ? out->data : plane(L.a[k]);
    if (k == 0) {
      K.label = label;
      K.has_post = post != nullptr;
      if (post) K.exposure = post->exposure, K.reinhard = post->reinhard;
    }
    e = lrp::launch_multiband_collapse(K, C, stream);
    if (e != hipSuccess) return hip_fail(e, "multi-band collapse kernel launch");
  }
  if (packed) { // level 0, into the packed output
    lrp::MbCollapsePackedParams K;
    std::memset(&K, 0, sizeof(K));
    K.a = plane(L.a[0]), K.s = plane(L.s[0]);
    K.w = L.w[0], K.h = L.h[0];
    K.top = B == 0;
    if (!K.top) K.cr = plane(L.a[1]), K.cw = L.w[1], K.ch = L.h[1];
    K.wrap = wrap;
    K.dst = out->data;
    K.label = label;
    K.has_post = post != nullptr;
    if (post) K.exposure = post->exposure, K.reinhard = post->reinhard;
    K.out_channels = packed->out_pch, K.out_format = packed->out_format, K.out_fill = packed->out_fill;
    e = lrp::launch_mb_collapse_packed(K, C, packed->device, stream);
    if (e != hipSuccess) return hip_fail(e, "packed multi-band collapse kernel launch");
  }
  return LRP_OK;
}

// Grow-only device / pinned buffer.
struct Buffer {
  void *ptr = nullptr;
  size_t cap = 0;
  bool pinned_host = false;
  int reserve(size_t bytes) {
    if (bytes <= cap) return LRP_OK;
    release();
    hipError_t e = pinned_host ? hipHostMalloc(&ptr, bytes, hipHostMallocDefault) : hipMalloc(&ptr, bytes);
    if (e == hipErrorOutOfMemory && !pinned_host) { // the geometry cache of THIS GPU holds what it holds for speed only: give it back, once
      (void)hipGetLastError();
      int dev = -1;
      if (hipGetDevice(&dev) == hipSuccess) lrp::geo_release_device(dev); // (the allocation is on the calling thread's current device)
      e = hipMalloc(&ptr, bytes);
    }
    if (e != hipSuccess) {
      ptr = nullptr;
      cap = 0;
      return hip_fail(e, pinned_host ? "hipHostMalloc" : "hipMalloc");
    }
    cap = bytes;
    return LRP_OK;
  }
  void release() {
    if (ptr) {
      if (pinned_host)
        (void)hipHostFree(ptr);
      else
        (void)hipFree(ptr);
    }
    ptr = nullptr;
    cap = 0;
  }
};

// One image in flight: device source + destination and the events that hand it
// from the upload stream to the compute stream to the download stream.
struct Slot {
  Buffer d_in, d_out;
  Buffer d_in_packed, d_out_packed; // the frame in its file format (lrp_context_submit_packed)
  hipEvent_t uploaded = nullptr, computed = nullptr, downloaded = nullptr;
  bool used = false;
};

} // namespace

// Three-stage pipeline: H2D on `up`, kernels on `run`, D2H on `down`, so that the
// upload of image i+1, the kernel of image i and the download of image i-1 use
// both PCIe directions and the GPU at the same time (a stream per image does not:
// its own H2D -> kernel -> D2H chain keeps one DMA direction idle).
struct lrp_context {
  std::mutex mutex; // submissions from several host threads are serialised
  int device = 0;
  hipStream_t up = nullptr, run = nullptr, down = nullptr;
  // Consecutive images alternate between two compute streams (contexts with more than one slot): the tail of image i's
  // launch — the last 6 % of a single 4K launch run with the wave slots draining — overlaps the head of image i + 1's.
  // Same-box A/B, single launches of one geometry, wall time per launch: headline 115.2 -> 107.7 us, equirect -> rect
  // 109.0 -> 102.0, equirect -> fisheye rotated 146.4 -> 138.1 (three streams: no further gain).
  hipStream_t run2 = nullptr;
  unsigned run_next = 0;
  std::vector<Slot> slots;
  size_t next = 0;
  int outside_mask = 0, outside_alpha = -1; // lrp_context_set_outside: the coverage kernel behind every reprojection (off)
};

extern "C" {

int lrp_abi_version(void) { return LRP_ABI_VERSION; }

int lrp_lens_extensions(int mask) {
  if (mask < 0) return g_lens_ext.load(std::memory_order_relaxed);
  return g_lens_ext.exchange(mask & (LRP_LENS_EXT_EQUISOLID | LRP_LENS_EXT_STEREOGRAPHIC), std::memory_order_relaxed);
}

int lrp_sampler_extensions(int mask) {
  if (mask < 0) return g_sampler_ext.load(std::memory_order_relaxed);
  return g_sampler_ext.exchange(mask & LRP_SAMPLER_EXT_LANCZOS3, std::memory_order_relaxed);
}

int lrp_debug_kernel(int choice) {
  if (choice < 0 || choice > 3) return kernel_choice();
  return g_knobs[kKnobKernel].exchange(choice, std::memory_order_relaxed);
}

int lrp_debug_set(const char *name, int value) {
  if (!name) return -1;
  for (int k = 0; k < kKnobCount; ++k)
    if (std::strcmp(name, kKnobs[k].name) == 0) {
      if (value < kKnobs[k].lo || value > kKnobs[k].hi) return knob(k);
      return g_knobs[k].exchange(value, std::memory_order_relaxed);
    }
  return -1;
}

void lrp_release_cached_tables(void) {
  lrp::geo_release_all();
  lrp::release_output_tables();
}

int lrp_geometry_cache_configure(long long max_bytes, int min_sightings) {
  lrp::geo_configure(max_bytes, min_sightings);
  return LRP_OK;
}

void lrp_geometry_cache_stats(lrp_geometry_cache_info *out) {
  if (!out) return;
  lrp::GeoStats st{};
  lrp::geo_stats(&st);
  out->bytes = st.bytes;
  out->max_bytes = st.max_bytes;
  out->entries = st.entries;
  out->fills = st.fills;
  out->hits = st.hits;
  out->bypasses = st.bypasses;
  out->evictions = st.evictions;
}

int lrp_device_count(void) { return device_count_cached(); }

const char *lrp_strerror(int status) {
  switch (status) {
  case LRP_OK: return "ok";
  case LRP_ERR_OUTPUT_LENS: return "Output lens type not supported.";
  case LRP_ERR_INPUT_LENS: return "Input lens type not supported.";
  case LRP_ERR_INTERPOLATION: return "Interpolation method not supported.";
  case LRP_ERR_CHANNELS: return "channel count mismatch or unsupported";
  case LRP_ERR_BAD_DIMS: return "bad image dimensions";
  case LRP_ERR_NULL: return "null pointer";
  case LRP_ERR_NO_DEVICE: return "no usable HIP device";
  case LRP_ERR_HIP: return "HIP runtime error";
  case LRP_ERR_OOM: return "out of memory";
  case LRP_ERR_BAD_ARG: return "bad argument";
  default: return "unknown status";
  }
}

const char *lrp_last_error(void) { return g_last_error.c_str(); }

int lrp_reproject_device(const lrp_image *in, lrp_image *out, int num_samples, int interpolation,
                         const float *rotation, const lrp_post *post, int device, void *stream) {
  int st = validate(in, out, interpolation, true, true);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_reproject(in, out, num_samples, interpolation, rotation, post, device, (hipStream_t)stream);
}

int lrp_reproject_rows_device(const lrp_image *in, lrp_image *out, int num_samples, int interpolation, const float *rotation,
                              const lrp_post *post, int row_first, int row_count, int device, void *stream) {
  int st = validate(in, out, interpolation, true, true);
  if (st != LRP_OK) return st;
  if (row_first < 0 || row_count < 0 || row_first > out->height - row_count)
    return fail(LRP_ERR_BAD_ARG, "row band outside the output image");
  st = select_device(device);
  if (st != LRP_OK) return st;
  if (row_count == 0) return LRP_OK;
  return enqueue_reproject(in, out, num_samples, interpolation, rotation, post, device, (hipStream_t)stream, 0, row_first, row_count);
}

int lrp_coverage_device(const lrp_image *in, const lrp_image *out, int num_samples, const float *rotation, uint8_t *coverage,
                        int mask_image, int alpha_channel, int device, void *stream) {
  int st = validate_coverage(in, out, num_samples, coverage != nullptr, mask_image, alpha_channel);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_coverage(in, out, num_samples, rotation, coverage, mask_image, alpha_channel, (hipStream_t)stream);
}

int lrp_compose_device(const lrp_image *ins, int n_in, const float *rotations, const lrp_image *out, int interpolation, int mode,
                       const lrp_post *post, uint8_t *count, int device, void *stream) {
  int st = validate_compose(ins, n_in, out, interpolation, mode);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_compose(ins, n_in, rotations, out, interpolation, mode, post, count, (hipStream_t)stream);
}

int lrp_compose_ss_device(const lrp_image *ins, int n_in, const float *rotations, const lrp_image *out, int num_samples, int interpolation,
                          int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage, int device, void *stream) {
  int st = validate_compose(ins, n_in, out, interpolation, mode);
  if (st != LRP_OK) return st;
  st = check_compose_samples(num_samples);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_compose_ss(ins, n_in, rotations, out, num_samples, interpolation, mode, post, count, coverage, (hipStream_t)stream);
}

int lrp_compose_cameras_device(const lrp_camera *cams, int n_in, const float *rotations, const lrp_image *out, int num_samples,
                               int interpolation, int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage, int device, void *stream) {
  int st = validate_compose_cameras(cams, n_in, out, num_samples, interpolation, mode);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_compose_cameras(cams, n_in, rotations, out, num_samples, interpolation, mode, post, count, coverage, (hipStream_t)stream);
}

int lrp_camera_overlap_device(const lrp_camera *cams, int n_in, const float *rotations, const lrp_image *out, float lo, float hi,
                              uint64_t *stats, int device, void *stream) {
  // (no mode and a fixed sampler: items 1 and 4 see values that pass)
  int st = validate_cameras_and_output(cams, n_in, out, LRP_BILINEAR, LRP_COMPOSE_FIRST, false, false, nullptr);
  if (st != LRP_OK) return st;
  st = check_overlap(stats, lo, hi);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_camera_overlap(cams, n_in, rotations, out, lo, hi, stats, (hipStream_t)stream);
}

// Host only, in double: the normal equations of Brown and Lowe's gain compensation over the cameras with N_kk > 0, solved by
// Gaussian elimination with partial pivoting.
int lrp_camera_gains(const uint64_t *stats, int n_in, float sigma_n, float sigma_g, float *gains) {
  if (!stats || !gains) return fail(LRP_ERR_NULL, "null stats or gains");
  if (n_in < 1 || n_in > LRP_COMPOSE_MAX_SOURCES) return fail(LRP_ERR_BAD_ARG, "n_in must be 1 .. " + std::to_string(LRP_COMPOSE_MAX_SOURCES));
  if (!std::isfinite(sigma_n) || !(sigma_n > 0.0f) || !std::isfinite(sigma_g) || !(sigma_g > 0.0f))
    return fail(LRP_ERR_BAD_ARG, "sigma_n and sigma_g must be finite and positive");
  constexpr int M = LRP_COMPOSE_MAX_SOURCES;
  const auto N = [&](int i, int j) { return (double)stats[(i * M + j) * 2]; };
  const auto I = [&](int i, int j) {
    const uint64_t n = stats[(i * M + j) * 2];
    return n == 0 ? 0.0 : (double)stats[(i * M + j) * 2 + 1] / (65536.0 * (double)n);
  };
  int active[M], m = 0;
  for (int k = 0; k < n_in; ++k) {
    gains[k] = 1.0f;
    if (stats[(k * M + k) * 2] > 0) active[m++] = k;
  }
  if (m == 0) return LRP_OK;
  const double inv_n2 = 1.0 / ((double)sigma_n * (double)sigma_n), inv_g2 = 1.0 / ((double)sigma_g * (double)sigma_g);
  double A[M][M + 1]; // the augmented matrix [A | b]
  for (int r = 0; r < m; ++r) {
    const int k = active[r];
    double diag = 0.0, prior = 0.0;
    for (int c = 0; c < m; ++c) {
      const int j = active[c];
      prior += N(k, j) * inv_g2;
      if (j == k) continue;
      diag += 2.0 * N(k, j) * I(k, j) * I(k, j) * inv_n2;
      A[r][c] = -2.0 * N(k, j) * I(k, j) * I(j, k) * inv_n2;
    }
    A[r][r] = diag + prior;
    A[r][m] = prior;
  }
  for (int p = 0; p < m; ++p) { // elimination with partial pivoting
    int best = p;
    for (int r = p + 1; r < m; ++r)
      if (std::fabs(A[r][p]) > std::fabs(A[best][p])) best = r;
    if (A[best][p] == 0.0) return fail(LRP_ERR_BAD_ARG, "the gain system is singular");
    if (best != p)
      for (int c = 0; c <= m; ++c) std::swap(A[p][c], A[best][c]);
    for (int r = p + 1; r < m; ++r) {
      const double f = A[r][p] / A[p][p];
      for (int c = p; c <= m; ++c) A[r][c] -= f * A[p][c];
    }
  }
  double g[M];
  for (int r = m - 1; r >= 0; --r) {
    double s = A[r][m];
    for (int c = r + 1; c < m; ++c) s -= A[r][c] * g[c];
    g[r] = s / A[r][r];
  }
  for (int r = 0; r < m; ++r) gains[active[r]] = (float)g[r];
  return LRP_OK;
}

int lrp_compose_cameras_gain_device(const lrp_camera *cams, int n_in, const float *rotations, const float *gains, const lrp_image *out,
                                    int num_samples, int interpolation, int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage,
                                    int device, void *stream) {
  int st = validate_cameras_and_output(cams, n_in, out, interpolation, mode, true, true, gains);
  if (st != LRP_OK) return st;
  st = check_gains(gains, n_in);
  if (st != LRP_OK) return st;
  st = check_compose_samples(num_samples);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_compose_cameras_gain(cams, n_in, rotations, gains, out, num_samples, interpolation, mode, post, count, coverage,
                                      (hipStream_t)stream);
}

int lrp_multiband_scratch_bytes(int width, int height, int channels, int num_bands, size_t *bytes) {
  if (!bytes) return fail(LRP_ERR_NULL, "null bytes");
  if (width < 1 || height < 1) return fail(LRP_ERR_BAD_DIMS, "image dimensions must be positive");
  if (channels < 1 || channels > lrp::kMultibandMaxChannels) return fail(LRP_ERR_CHANNELS, "channels of a multi-band call must be 1 .. 4");
  if (num_bands < 0 || num_bands > LRP_MULTIBAND_MAX_BANDS) return fail(LRP_ERR_BAD_ARG, "num_bands must be 0 .. " + std::to_string(LRP_MULTIBAND_MAX_BANDS));
  *bytes = lrp::multiband_layout(width, height, channels, num_bands).total;
  return LRP_OK;
}

int lrp_compose_cameras_multiband_device(const lrp_camera *cams, int n_in, const float *rotations, const float *gains, const lrp_image *out,
                                         int interpolation, int num_bands, const lrp_post *post, uint8_t *count, uint8_t *label, void *scratch,
                                         size_t scratch_bytes, int device, void *stream) {
  int st = validate_multiband(cams, n_in, gains, out, interpolation, num_bands, scratch, scratch_bytes);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_multiband(cams, n_in, rotations, gains, out, interpolation, num_bands, post, count, label, scratch, nullptr, (hipStream_t)stream);
}

int lrp_camera_view_device(const lrp_camera *cams, int n_in, const float *rotations, const lrp_camera *target, float *out_data, int channels,
                           int num_samples, int interpolation, int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage, int device,
                           void *stream) {
  int st = validate_camera_view(cams, n_in, target, out_data, channels, num_samples, interpolation, mode);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_camera_view(cams, n_in, rotations, target, out_data, channels, num_samples, interpolation, mode, post, count, coverage,
                             (hipStream_t)stream);
}

// Host only: camera_unproject (lrp_camera_inverse.h), the function the kernel calls, on the host.
int lrp_camera_unproject(const lrp_camera *cam, const float *uv, int n, float *rays, uint8_t *has_ray) {
  if (!cam || !uv || !rays) return fail(LRP_ERR_NULL, "null camera, uv or rays");
  if (n < 0) return fail(LRP_ERR_BAD_ARG, "n must be >= 0");
  lrp_camera c = *cam;
  c.width = c.height = 1; // (the size is not looked at; what is left of the checks is LRP_ERR_BAD_ARG)
  const int st = validate_camera(c, "camera: ", 1, false);
  if (st != LRP_OK) return st;
  lrp::CameraSource T;
  std::memset(&T, 0, sizeof(T));
  pack_camera(T, c);
  for (int j = 0; j < n; ++j) {
    float *r = rays + 3 * (size_t)j;
    const float u = uv[2 * (size_t)j], v = uv[2 * (size_t)j + 1];
    const bool ok = c.model == LRP_CAMERA_FISHEYE ? lrp::camera_unproject<lrp::kCameraFisheye>(T, u, v, r[0], r[1], r[2])
                                                  : lrp::camera_unproject<lrp::kCameraBrown>(T, u, v, r[0], r[1], r[2]);
    if (has_ray) has_ray[j] = ok ? 1 : 0;
  }
  return LRP_OK;
}

// Host only, in double.  g(x) = x * (1 + c0 x^2 + c1 x^4 + c2 x^6 + c3 x^8) is scanned upwards in steps of h while it increases; the
// step that stops increasing brackets the turning point between the sample before it and the sample after it, and the root of g'
// in that bracket is closed in on by bisection from below, so that the result never exceeds the turning point.
int lrp_camera_limit(const lrp_camera *cam, float *limit) {
  if (!cam || !limit) return fail(LRP_ERR_NULL, "null camera or limit");
  if (cam->model != LRP_CAMERA_BROWN && cam->model != LRP_CAMERA_FISHEYE) return fail(LRP_ERR_BAD_ARG, "unknown camera model");
  double c[4];
  const int used = camera_radial(*cam, c);
  for (int j = 0; j < used; ++j)
    if (!std::isfinite(cam->k[j])) return fail(LRP_ERR_BAD_ARG, "k[" + std::to_string(j) + "] is not finite");
  const bool brown = cam->model == LRP_CAMERA_BROWN;
  const double x_max = brown ? 16.0 : M_PI;
  const int steps = brown ? 16 * 1024 : 4096;
  const double h = x_max / steps;
  const auto g = [&](double x) {
    const double x2 = x * x;
    return x * (1.0 + x2 * (c[0] + x2 * (c[1] + x2 * (c[2] + x2 * c[3]))));
  };
  const auto dg = [&](double x) {
    const double x2 = x * x;
    return 1.0 + x2 * (3.0 * c[0] + x2 * (5.0 * c[1] + x2 * (7.0 * c[2] + x2 * (9.0 * c[3]))));
  };
  int j = 0;
  while (j < steps && g((j + 1) * h) > g(j * h)) ++j;
  if (j == steps) { // increases all the way
    *limit = brown ? INFINITY : (float)M_PI; // (the float atan2f returns for the ray straight backwards)
    return LRP_OK;
  }
  double lo = j > 0 ? (j - 1) * h : 0.0, hi = (j + 1) * h; // g' > 0 at lo (or lo == 0, where g' == 1); the turning point is in [lo, hi]
  if (dg(lo) > 0.0 && !(dg(hi) > 0.0))
    for (int it = 0; it < 64; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (dg(mid) > 0.0)
        lo = mid;
      else
        hi = mid;
    }
  const double v = brown ? lo * lo : lo;
  float f = (float)v;
  if ((double)f > v) f = std::nextafter(f, 0.0f); // round down
  *limit = f;
  return LRP_OK;
}

int lrp_reproject_packed_device(const lrp_image *in, int in_format, int in_packed_channels, lrp_image *out, int out_format,
                                int out_packed_channels, unsigned out_fill, int num_samples, int interpolation, const float *rotation,
                                const lrp_post *post, int device, void *stream) {
  int st = validate_packed(in, in_format, in_packed_channels, out, out_format, out_packed_channels, interpolation);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_packed(in, in_format, in_packed_channels, out, out_format, out_packed_channels, out_fill, num_samples, interpolation,
                        rotation, post, device, (hipStream_t)stream);
}

int lrp_compose_packed_device(const lrp_image *ins, int n_in, int in_format, int in_packed_channels, const float *rotations,
                              const lrp_image *out, int out_format, int out_packed_channels, unsigned out_fill, int interpolation, int mode,
                              const lrp_post *post, uint8_t *count, int device, void *stream) {
  int st = validate_compose_packed(ins, n_in, in_format, in_packed_channels, out, out_format, out_packed_channels, interpolation, mode);
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_compose_packed(ins, n_in, in_format, in_packed_channels, rotations, out, out_format, out_packed_channels, out_fill,
                                interpolation, mode, post, count, device, (hipStream_t)stream);
}

int lrp_compose_cameras_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels, const float *rotations,
                                      const float *gains, const lrp_image *out, int out_format, int out_packed_channels, unsigned out_fill,
                                      int num_samples, int interpolation, int mode, const lrp_post *post, uint8_t *count, uint8_t *coverage,
                                      int device, void *stream) {
  int st = validate_cameras_and_output(cams, n_in, out, interpolation, mode, true, false, nullptr);
  if (st != LRP_OK) return st;
  if (gains) {
    st = check_gains(gains, n_in);
    if (st != LRP_OK) return st;
  }
  st = check_compose_samples(num_samples);
  if (st != LRP_OK) return st;
  st = validate_cameras_packed(cams, n_in, in_format, in_packed_channels, out, true, out_format, out_packed_channels, "lrp_compose_cameras_packed_device takes",
                               "lrp_compose_cameras_device or lrp_compose_cameras_gain_device, then lrp_encode_pixels_device");
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_compose_cameras_packed(cams, n_in, in_format, in_packed_channels, rotations, gains, out, out_format, out_packed_channels,
                                        out_fill, num_samples, interpolation, mode, post, count, coverage, device, (hipStream_t)stream);
}

int lrp_compose_cameras_multiband_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels, const float *rotations,
                                                const float *gains, const lrp_image *out, int out_format, int out_packed_channels,
                                                unsigned out_fill, int interpolation, int num_bands, const lrp_post *post, uint8_t *count,
                                                uint8_t *label, void *scratch, size_t scratch_bytes, int device, void *stream) {
  int st = validate_multiband(cams, n_in, gains, out, interpolation, num_bands, scratch, scratch_bytes);
  if (st != LRP_OK) return st;
  // (C <= 4 has passed: the packed calls' own channel item cannot fire)
  st = validate_cameras_packed(cams, n_in, in_format, in_packed_channels, out, true, out_format, out_packed_channels,
                               "lrp_compose_cameras_multiband_packed_device takes", "lrp_compose_cameras_multiband_device, then lrp_encode_pixels_device");
  if (st != LRP_OK) return st;
  // a camera's level-0 layer is a float32 image of C samples per pixel in the scratch, written by the packed camera kernel
  if (!packed_addressable(*out, LRP_PIXEL_F32, out->channels))
    return fail(LRP_ERR_BAD_DIMS, "the float32 level-0 layer of a packed multi-band call, width x height x channels x 4 bytes, must not exceed 2^31 bytes "
                                  "(the packed camera kernels form 32-bit byte offsets)");
  st = select_device(device);
  if (st != LRP_OK) return st;
  const MultibandPacked packed = {in_format, in_packed_channels, out_format, out_packed_channels, out_fill, device};
  return enqueue_multiband(cams, n_in, rotations, gains, out, interpolation, num_bands, post, count, label, scratch, &packed, (hipStream_t)stream);
}

int lrp_camera_overlap_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels, const float *rotations,
                                     const lrp_image *out, float lo, float hi, uint64_t *stats, int device, void *stream) {
  // (no mode and a fixed sampler: items 1 and 4 see values that pass)
  int st = validate_cameras_and_output(cams, n_in, out, LRP_BILINEAR, LRP_COMPOSE_FIRST, false, false, nullptr);
  if (st != LRP_OK) return st;
  st = check_overlap(stats, lo, hi);
  if (st != LRP_OK) return st;
  st = validate_cameras_packed(cams, n_in, in_format, in_packed_channels, out, false, 0, 0, "lrp_camera_overlap_packed_device takes", "lrp_camera_overlap_device");
  if (st != LRP_OK) return st;
  st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_camera_overlap_packed(cams, n_in, in_format, in_packed_channels, rotations, out, lo, hi, stats, device, (hipStream_t)stream);
}

namespace {
// Side streams of lrp_reproject_multi_device, per device, created on first use and kept.
constexpr int kMaxSide = kMaxSideStreams;
struct MultiFork {
  std::mutex busy; // one fork / join being enqueued at a time per device (the events are re-recorded by every call)
  hipStream_t side[kMaxSide] = {};
  hipEvent_t forked = nullptr, joined[kMaxSide] = {};
};
std::mutex g_fork_registry_mutex;
std::map<int, std::unique_ptr<MultiFork>> g_forks;
MultiFork *multi_fork(int device) { // null if the streams / events cannot be created (the caller then stays on one stream)
  std::lock_guard<std::mutex> lock(g_fork_registry_mutex);
  std::unique_ptr<MultiFork> &slot = g_forks[device];
  if (!slot) {
    std::unique_ptr<MultiFork> f(new MultiFork);
    bool ok = hipEventCreateWithFlags(&f->forked, hipEventDisableTiming) == hipSuccess;
    for (int k = 0; k < kMaxSide && ok; ++k)
      ok = hipStreamCreateWithFlags(&f->side[k], hipStreamNonBlocking) == hipSuccess &&
           hipEventCreateWithFlags(&f->joined[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      return nullptr;
    }
    slot = std::move(f);
  }
  return slot.get();
}
// Side streams lrp_reproject_multi_device deals its launches over besides the caller's (lrp_debug_set("multi_fork", n);
// 0 keeps every launch on the caller's stream; default 1 — measured best, 588 -> 509 us per 8192^2 -> 6 x 2048^2 cubemap; 2-3: 522, 5: 549).
int multi_fork_lanes() { return knob(kKnobMultiFork); }

} // namespace

int lrp_reproject_multi_device(const lrp_image *in, lrp_image *outs, int n_out, int num_samples,
                               int interpolation, const float *rotations, const lrp_post *post, int device,
                               void *stream) {
  if (n_out < 0 || (n_out > 0 && !outs)) return fail(LRP_ERR_BAD_ARG, "bad output array");
  for (int i = 0; i < n_out; ++i) {
    int st = validate(in, &outs[i], interpolation, true, true);
    if (st != LRP_OK) return st;
  }
  int st = select_device(device);
  if (st != LRP_OK) return st;
  // The launches are independent (one source, disjoint outputs) and each is short (a 2048^2 cubemap face: 70-150 us, one
  // or two rounds of wavefronts): dealt over the caller's stream and two side streams the tail of one launch overlaps
  // the head of the next.  Fork / join by events; everything stays ordered behind the caller's earlier work and in front
  // of its later work.  (Not while the caller's stream is being captured into a graph, and not for a single output.)
  MultiFork *fork = nullptr;
  std::unique_lock<std::mutex> fork_lock;
  hipStream_t lanes[kMaxSide + 1];
  int n_lanes = 1;
  lanes[0] = (hipStream_t)stream;
  const int want_side = std::min(multi_fork_lanes(), n_out - 1);
  bool forked = false;
  if (want_side > 0) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap == hipStreamCaptureStatusNone && (fork = multi_fork(device)) != nullptr) {
      fork_lock = std::unique_lock<std::mutex>(fork->busy);
      bool ok = hipEventRecord(fork->forked, (hipStream_t)stream) == hipSuccess;
      for (int k = 0; k < want_side && ok; ++k) ok = hipStreamWaitEvent(fork->side[k], fork->forked, 0) == hipSuccess;
      if (ok) {
        for (int k = 0; k < want_side; ++k) lanes[n_lanes++] = fork->side[k];
        forked = true;
      } else { // (side streams that already wait on the event just wait for the caller's earlier work: harmless)
        (void)hipGetLastError();
      }
    }
  }
  int result = LRP_OK;
  for (int i = 0; i < n_out && result == LRP_OK; ++i)
    result = enqueue_reproject(in, &outs[i], num_samples, interpolation, rotations ? rotations + 9 * i : nullptr, post, device, lanes[i % n_lanes]);
  if (fork != nullptr && forked) // join, whatever happened: the caller's stream continues behind the side streams
    for (int k = 0; k + 1 < n_lanes; ++k)
      if (hipEventRecord(fork->joined[k], fork->side[k]) != hipSuccess || hipStreamWaitEvent((hipStream_t)stream, fork->joined[k], 0) != hipSuccess) {
        const hipError_t e = hipGetLastError();
        (void)hipStreamSynchronize(fork->side[k]);
        if (result == LRP_OK) result = hip_fail(e == hipSuccess ? hipErrorUnknown : e, "join of lrp_reproject_multi_device");
      }
  return result;
}

namespace {
// Per participant of lrp_reproject_multi: a stream and grow-only buffers, kept for the next call.  A participant is a
// (device, occurrence) pair — a device list may name one GPU several times (tests on a one-GPU box do) — and is locked
// for the duration of a job, so jobs on disjoint device sets run concurrently and jobs that share a GPU queue up on it.
struct MultiPeer {
  int device = -1;
  std::mutex busy;
  hipStream_t stream = nullptr;
  hipEvent_t source_ready = nullptr;
  Buffer src, out;
};
std::mutex g_multi_registry_mutex; // guards the map only, never held while a job runs
std::map<std::pair<int, int>, std::unique_ptr<MultiPeer>> g_multi_peers;

MultiPeer *multi_peer(int device, int occurrence) {
  std::lock_guard<std::mutex> lock(g_multi_registry_mutex);
  std::unique_ptr<MultiPeer> &slot = g_multi_peers[{device, occurrence}];
  if (!slot) {
    slot.reset(new MultiPeer);
    slot->device = device;
  }
  return slot.get();
}
} // namespace

int lrp_reproject_multi(const lrp_image *in, lrp_image *outs, int n_out, int num_samples, int interpolation,
                        const float *rotations, const lrp_post *post, const int *devices, int n_devices) {
  if (n_out < 0 || (n_out > 0 && !outs) || !devices || n_devices < 1 || n_devices > 64)
    return fail(LRP_ERR_BAD_ARG, "bad output array or device list");
  for (int i = 0; i < n_out; ++i) {
    int st = validate(in, &outs[i], interpolation, true, true);
    if (st != LRP_OK) return st;
  }
  for (int d = 0; d < n_devices; ++d) {
    int st = select_device(devices[d]);
    if (st != LRP_OK) return st;
  }
  if (n_out == 0 || num_samples <= 0) return LRP_OK;
  // participants in list order; locked in (device, occurrence) order so that two jobs never wait for each other
  std::vector<MultiPeer *> peers((size_t)n_devices);
  for (int d = 0; d < n_devices; ++d) {
    int occurrence = 0;
    for (int e = 0; e < d; ++e) occurrence += devices[e] == devices[d];
    peers[(size_t)d] = multi_peer(devices[d], occurrence);
  }
  std::vector<MultiPeer *> order(peers);
  std::sort(order.begin(), order.end(), std::less<MultiPeer *>()); // stable addresses (map of unique_ptr): any total order will do
  std::vector<std::unique_lock<std::mutex>> locks;
  for (MultiPeer *p : order) locks.emplace_back(p->busy);

  const size_t in_bytes = image_bytes(*in);
  // With at least as many outputs as participants whole outputs are dealt round-robin (output i -> participant i % n): a
  // whole image keeps the kernels that share work between mirror images and the geometry cache.  With fewer outputs than
  // participants every participant renders band d of every output (rows are independent, src/reproject.cpp:284).  Either
  // way a participant's output buffer holds its pieces back to back.
  const bool whole_outputs = n_out >= n_devices;
  auto band = [&](int i, int d, int &first, int &count) {
    const lrp_image &o = outs[i];
    if (whole_outputs) {
      first = 0;
      count = (i % n_devices == d) ? o.height : 0;
      return;
    }
    first = (int)((long long)o.height * d / n_devices);
    count = (int)((long long)o.height * (d + 1) / n_devices) - first;
  };
  // Everything that can fail after the first asynchronous copy has been enqueued goes through `result` and falls
  // through to the synchronisation of every participant's stream below: no copy out of in->data or into outs[i].data
  // is in flight when this function returns, whatever happened.
  int result = LRP_OK;
  auto hip_ok = [&](hipError_t e, const char *what) {
    if (e != hipSuccess && result == LRP_OK) result = hip_fail(e, what);
    return e == hipSuccess && result == LRP_OK;
  };
  // Where a participant's source lives: the first participant on a GPU holds the copy of that GPU (`holder[d] == d`), later
  // occurrences of the same GPU read it in place.  The holders receive it in a binary tree: holder k (k-th distinct GPU)
  // copies from holder k - 2^floor(log2 k) — after round r, 2^r GPUs hold the source and every one of them feeds another,
  // each over its own xGMI link (seven copies out of one root share that root's links and its HBM read bandwidth: 805 MB x 7).
  std::vector<int> holder((size_t)n_devices), holders;
  for (int d = 0; d < n_devices; ++d) {
    holder[(size_t)d] = d;
    for (int e = 0; e < d; ++e)
      if (devices[e] == devices[d]) {
        holder[(size_t)d] = e;
        break;
      }
    if (holder[(size_t)d] == d) holders.push_back(d);
  }
  for (int d = 0; d < n_devices && result == LRP_OK; ++d) {
    MultiPeer &p = *peers[(size_t)d];
    if (!hip_ok(hipSetDevice(p.device), "hipSetDevice")) break;
    if (!p.stream && !hip_ok(hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking), "hipStreamCreateWithFlags")) break;
    if (!p.source_ready && !hip_ok(hipEventCreateWithFlags(&p.source_ready, hipEventDisableTiming), "hipEventCreateWithFlags")) break;
    size_t out_bytes = 0;
    for (int i = 0; i < n_out; ++i) {
      int first, count;
      band(i, d, first, count);
      out_bytes += (size_t)count * (size_t)outs[i].width * (size_t)outs[i].channels * 4u;
    }
    if (holder[(size_t)d] == d) result = p.src.reserve(in_bytes);
    if (result == LRP_OK) result = p.out.reserve(out_bytes ? out_bytes : 4);
  }
  // the source: host -> devices[0] once, then device to device down the tree
  MultiPeer &root = *peers[0];
  if (result == LRP_OK && hip_ok(hipSetDevice(root.device), "hipSetDevice") &&
      hip_ok(hipMemcpyAsync(root.src.ptr, in->data, in_bytes, hipMemcpyHostToDevice, root.stream), "hipMemcpyAsync (source upload)"))
    hip_ok(hipEventRecord(root.source_ready, root.stream), "hipEventRecord");
  for (size_t k = 1; k < holders.size() && result == LRP_OK; ++k) {
    size_t top = 1;
    while (top * 2 <= k) top *= 2;
    MultiPeer &p = *peers[(size_t)holders[k]], &from = *peers[(size_t)holders[k - top]];
    if (!hip_ok(hipSetDevice(p.device), "hipSetDevice")) break;
    int can = 0;
    (void)hipDeviceCanAccessPeer(&can, p.device, from.device);
    if (can) {
      const hipError_t e = hipDeviceEnablePeerAccess(from.device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
      (void)hipGetLastError();
    }
    if (can) {
      if (hip_ok(hipStreamWaitEvent(p.stream, from.source_ready, 0), "hipStreamWaitEvent"))
        hip_ok(hipMemcpyPeerAsync(p.src.ptr, p.device, from.src.ptr, from.device, in_bytes, p.stream), "hipMemcpyPeerAsync");
    } else {
      hip_ok(hipMemcpyAsync(p.src.ptr, in->data, in_bytes, hipMemcpyHostToDevice, p.stream), "hipMemcpyAsync (second upload)");
    }
    if (result == LRP_OK) hip_ok(hipEventRecord(p.source_ready, p.stream), "hipEventRecord");
  }
  // later occurrences of a GPU wait for that GPU's copy
  for (int d = 0; d < n_devices && result == LRP_OK; ++d) {
    if (holder[(size_t)d] == d) continue;
    MultiPeer &p = *peers[(size_t)d];
    if (!hip_ok(hipSetDevice(p.device), "hipSetDevice")) break;
    hip_ok(hipStreamWaitEvent(p.stream, peers[(size_t)holder[(size_t)d]]->source_ready, 0), "hipStreamWaitEvent");
  }
  // bands: render into the participant's buffer at the band's own row offset (the kernels address whole images),
  // download each band to its rows of the host output
  for (int d = 0; d < n_devices && result == LRP_OK; ++d) {
    MultiPeer &p = *peers[(size_t)d];
    if (!hip_ok(hipSetDevice(p.device), "hipSetDevice")) break;
    size_t cursor = 0; // floats into p.out
    for (int i = 0; i < n_out && result == LRP_OK; ++i) {
      int first, count;
      band(i, d, first, count);
      if (count == 0) continue;
      const size_t row_floats = (size_t)outs[i].width * (size_t)outs[i].channels;
      lrp_image din = *in, dout = outs[i];
      din.data = (float *)peers[(size_t)holder[(size_t)d]]->src.ptr;
      // a virtual whole image whose rows [first, first + count) are the buffer's [cursor, ...): only those are written
      dout.data = (float *)p.out.ptr + cursor - (size_t)first * row_floats;
      result = enqueue_reproject(&din, &dout, num_samples, interpolation, rotations ? rotations + 9 * i : nullptr, post, p.device,
                                 p.stream, 0, first, count);
      if (result != LRP_OK) break;
      hip_ok(hipMemcpyAsync(outs[i].data + (size_t)first * row_floats, (float *)p.out.ptr + cursor, (size_t)count * row_floats * 4u,
                            hipMemcpyDeviceToHost, p.stream), "hipMemcpyAsync (band download)");
      cursor += (size_t)count * row_floats;
    }
  }
  // the one exit: every participant's stream drained, then the first error (if any)
  for (MultiPeer *p : peers) {
    if (!p->stream) continue;
    (void)hipSetDevice(p->device);
    const hipError_t e = hipStreamSynchronize(p->stream);
    if (e != hipSuccess && result == LRP_OK) result = hip_fail(e, "hipStreamSynchronize");
  }
  return result;
}

int lrp_reproject_batch_device(const lrp_image *ins, lrp_image *outs, int n, int num_samples, int interpolation,
                               const float *rotation, const lrp_post *post, int device, void *stream) {
  if (n < 0 || (n > 0 && (!ins || !outs))) return fail(LRP_ERR_BAD_ARG, "bad image arrays");
  if (n == 0) return LRP_OK;
  for (int i = 0; i < n; ++i) {
    int st = validate(&ins[i], &outs[i], interpolation, true, true);
    if (st != LRP_OK) return st;
    const bool same = ins[i].width == ins[0].width && ins[i].height == ins[0].height && ins[i].channels == ins[0].channels &&
                      outs[i].width == outs[0].width && outs[i].height == outs[0].height &&
                      std::memcmp(&ins[i].lens, &ins[0].lens, sizeof(lrp_lens)) == 0 &&
                      std::memcmp(&outs[i].lens, &outs[0].lens, sizeof(lrp_lens)) == 0;
    if (!same) return fail(LRP_ERR_BAD_ARG, "the images of a batch must share sizes, channel count and lenses");
  }
  int st = select_device(device);
  if (st != LRP_OK) return st;
  return enqueue_reproject(ins, outs, num_samples, interpolation, rotation, post, device, (hipStream_t)stream, n);
}

int lrp_post_process_device(lrp_image *img, float exposure, float reinhard, int device, void *stream) {
  if (!img || !img->data) return fail(LRP_ERR_NULL, "null image");
  if (img->width < 1 || img->height < 1 || img->channels < 1) return fail(LRP_ERR_BAD_DIMS, "bad image dimensions");
  if (!image_addressable(*img)) return fail(LRP_ERR_BAD_DIMS, "image too large (more than 2^31 floats)");
  int st = select_device(device);
  if (st != LRP_OK) return st;
  hipError_t e = lrp::launch_post_process(img->data, (uint32_t)img->width * (uint32_t)img->height, img->channels,
                                          exposure, reinhard, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "post_process kernel launch");
  return LRP_OK;
}

int lrp_context_create(lrp_context **ctx, int device, int n_streams) {
  if (!ctx || n_streams < 1 || n_streams > 64) return fail(LRP_ERR_BAD_ARG, "bad context arguments");
  int st = select_device(device);
  if (st != LRP_OK) return st;
  lrp_context *c = new (std::nothrow) lrp_context;
  if (!c) return fail(LRP_ERR_OOM, "host allocation failed");
  c->device = device;
  c->slots.resize((size_t)n_streams);
  hipError_t e = hipStreamCreateWithFlags(&c->up, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->run, hipStreamNonBlocking);
  if (e == hipSuccess && n_streams > 1) e = hipStreamCreateWithFlags(&c->run2, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->down, hipStreamNonBlocking);
  for (auto &s : c->slots) {
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.computed, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.downloaded, hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    lrp_context_destroy(c);
    return hip_fail(e, "stream / event creation");
  }
  *ctx = c;
  return LRP_OK;
}

void lrp_context_destroy(lrp_context *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (hipStream_t st : {ctx->up, ctx->run, ctx->run2, ctx->down})
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  for (auto &s : ctx->slots) {
    for (hipEvent_t ev : {s.uploaded, s.computed, s.downloaded})
      if (ev) (void)hipEventDestroy(ev);
    s.d_in.release();
    s.d_out.release();
    s.d_in_packed.release();
    s.d_out_packed.release();
  }
  delete ctx;
}

namespace {
// One image through the three-stage pipeline.  Formats LRP_PIXEL_F32 with packed channels == image
// channels: the host buffers are the kernels' own layout and are copied straight into / out of the
// slot's float buffers; otherwise the frame is uploaded as it is and converted on the device.
int submit_locked(lrp_context *ctx, const lrp_image *in, int in_format, int in_pch, lrp_image *out, int out_format,
                  int out_pch, unsigned out_fill, int num_samples, int interpolation, const float *rotation,
                  const lrp_post *post, int *ticket) {
  const size_t index = ctx->next;
  Slot &s = ctx->slots[index];
  ctx->next = (ctx->next + 1) % ctx->slots.size();
  if (ticket) *ticket = (int)index;
  const size_t in_px = (size_t)in->width * (size_t)in->height, out_px = (size_t)out->width * (size_t)out->height;
  const size_t in_bytes = image_bytes(*in), out_bytes = image_bytes(*out);
  const bool in_plain = in_format == LRP_PIXEL_F32 && in_pch == in->channels;
  const bool out_plain = out_format == LRP_PIXEL_F32 && out_pch == out->channels;
  const size_t in_packed = in_plain ? 0 : in_px * lrp::pixel_bytes(in_format, in_pch);
  const size_t out_packed = out_plain ? 0 : out_px * lrp::pixel_bytes(out_format, out_pch);
  if (in_bytes > s.d_in.cap || out_bytes > s.d_out.cap || in_packed > s.d_in_packed.cap || out_packed > s.d_out_packed.cap) {
    // growing a buffer frees the old one: the slot's previous image must have drained
    if (s.used) LRP_HIP_TRY(hipEventSynchronize(s.downloaded));
    int st = s.d_in.reserve(in_bytes);
    if (st == LRP_OK) st = s.d_out.reserve(out_bytes);
    if (st == LRP_OK && in_packed) st = s.d_in_packed.reserve(in_packed);
    if (st == LRP_OK && out_packed) st = s.d_out_packed.reserve(out_packed);
    if (st != LRP_OK) return st;
  }
  // upload: the slot's source buffers are free once its previous kernels have run
  if (s.used) LRP_HIP_TRY(hipStreamWaitEvent(ctx->up, s.computed, 0));
  LRP_HIP_TRY(hipMemcpyAsync(in_plain ? s.d_in.ptr : s.d_in_packed.ptr, in->data, in_plain ? in_bytes : in_packed,
                             hipMemcpyHostToDevice, ctx->up));
  LRP_HIP_TRY(hipEventRecord(s.uploaded, ctx->up));
  // kernels: after the upload, and after the previous download has read the destination buffers
  const hipStream_t run = (ctx->run2 != nullptr && knob(kKnobContextStreams) != 0 && (ctx->run_next++ & 1u) != 0) ? ctx->run2 : ctx->run;
  LRP_HIP_TRY(hipStreamWaitEvent(run, s.uploaded, 0));
  if (s.used) LRP_HIP_TRY(hipStreamWaitEvent(run, s.downloaded, 0));
  if (!in_plain) {
    hipError_t e = lrp::launch_decode_pixels(s.d_in_packed.ptr, in_format, in_pch, (float *)s.d_in.ptr, in->channels, in_px,
                                             ctx->device, run);
    if (e != hipSuccess) return hip_fail(e, "pixel decode kernel launch");
  }
  lrp_image din = *in, dout = *out;
  din.data = (float *)s.d_in.ptr;
  dout.data = (float *)s.d_out.ptr;
  int st = enqueue_reproject(&din, &dout, num_samples, interpolation, rotation, post, ctx->device, run);
  if (st != LRP_OK) return st;
  if (ctx->outside_mask != 0 || ctx->outside_alpha != -1) { // lrp_context_set_outside
    st = enqueue_coverage(&din, &dout, num_samples, rotation, nullptr, ctx->outside_mask, ctx->outside_alpha, run);
    if (st != LRP_OK) return st;
  }
  if (!out_plain) {
    hipError_t e = lrp::launch_encode_pixels((const float *)s.d_out.ptr, out->channels, s.d_out_packed.ptr, out_format, out_pch,
                                             out_fill, out_px, ctx->device, run);
    if (e != hipSuccess) return hip_fail(e, "pixel encode kernel launch");
  }
  LRP_HIP_TRY(hipEventRecord(s.computed, run));
  // download
  LRP_HIP_TRY(hipStreamWaitEvent(ctx->down, s.computed, 0));
  LRP_HIP_TRY(hipMemcpyAsync(out->data, out_plain ? s.d_out.ptr : s.d_out_packed.ptr, out_plain ? out_bytes : out_packed,
                             hipMemcpyDeviceToHost, ctx->down));
  LRP_HIP_TRY(hipEventRecord(s.downloaded, ctx->down));
  s.used = true;
  return LRP_OK;
}
} // namespace

int lrp_context_submit_packed(lrp_context *ctx, const lrp_image *in, int in_format, int in_packed_channels, lrp_image *out,
                              int out_format, int out_packed_channels, unsigned out_fill, int num_samples,
                              int interpolation, const float *rotation, const lrp_post *post, int *ticket) {
  if (!ctx) return fail(LRP_ERR_NULL, "null context");
  if (ticket) *ticket = -1;
  int st = validate(in, out, interpolation, true, true);
  if (st != LRP_OK) return st;
  if (!format_ok(in_format) || !format_ok(out_format) || in_packed_channels < 1 || out_packed_channels < 1 ||
      in_packed_channels > 64 || out_packed_channels > 64)
    return fail(LRP_ERR_BAD_ARG, "bad pixel format or packed channel count");
  st = select_device(ctx->device);
  if (st != LRP_OK) return st;
  if (num_samples <= 0) return LRP_OK; // reference loop body never runs: output untouched
  std::lock_guard<std::mutex> lock(ctx->mutex);
  if (ctx->outside_mask != 0 || ctx->outside_alpha != -1) { // (before anything is enqueued)
    st = validate_coverage(in, out, num_samples, false, ctx->outside_mask, ctx->outside_alpha);
    if (st != LRP_OK) return st;
  }
  return submit_locked(ctx, in, in_format, in_packed_channels, out, out_format, out_packed_channels, out_fill, num_samples,
                       interpolation, rotation, post, ticket);
}

int lrp_context_submit(lrp_context *ctx, const lrp_image *in, lrp_image *out, int num_samples, int interpolation,
                       const float *rotation, const lrp_post *post) {
  if (!in || !out) return fail(LRP_ERR_NULL, "null image");
  return lrp_context_submit_packed(ctx, in, LRP_PIXEL_F32, in->channels, out, LRP_PIXEL_F32, out->channels, 0u, num_samples,
                                   interpolation, rotation, post, nullptr);
}

int lrp_context_set_outside(lrp_context *ctx, int mask_image, int alpha_channel) {
  if (!ctx) return fail(LRP_ERR_NULL, "null context");
  if (alpha_channel < -1) return fail(LRP_ERR_BAD_ARG, "alpha_channel must be -1 or a channel index");
  std::lock_guard<std::mutex> lock(ctx->mutex);
  ctx->outside_mask = mask_image != 0;
  ctx->outside_alpha = alpha_channel;
  return LRP_OK;
}

int lrp_context_wait_ticket(lrp_context *ctx, int ticket) {
  if (!ctx) return fail(LRP_ERR_NULL, "null context");
  if (ticket < 0) return LRP_OK; // nothing was enqueued (num_samples <= 0)
  if ((size_t)ticket >= ctx->slots.size()) return fail(LRP_ERR_BAD_ARG, "bad ticket");
  int st = select_device(ctx->device);
  if (st != LRP_OK) return st;
  hipEvent_t ev;
  {
    std::lock_guard<std::mutex> lock(ctx->mutex);
    ev = ctx->slots[(size_t)ticket].downloaded;
  }
  // (a later submission that re-used the slot has re-recorded the event behind this image's download
  // on the same stream: waiting for it waits for this image too)
  LRP_HIP_TRY(hipEventSynchronize(ev));
  return LRP_OK;
}

int lrp_context_wait(lrp_context *ctx) {
  if (!ctx) return fail(LRP_ERR_NULL, "null context");
  int st = select_device(ctx->device);
  if (st != LRP_OK) return st;
  int result = LRP_OK;
  std::lock_guard<std::mutex> lock(ctx->mutex);
  for (hipStream_t stream : {ctx->up, ctx->run, ctx->run2, ctx->down}) {
    if (!stream) continue;
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess && result == LRP_OK) result = hip_fail(e, "hipStreamSynchronize");
  }
  return result;
}

namespace {
// The synchronous host-buffer entry points borrow a single-stream context from
// a per-device pool (one per concurrent caller, reused afterwards), so repeated
// calls keep their device buffers and concurrent pool threads never share one.
// Pooled contexts live until process exit.
std::mutex g_pool_mutex;
std::vector<std::vector<lrp_context *>> g_pool; // [device] -> idle contexts

int borrow_context(int device, lrp_context **out) {
  int st = select_device(device);
  if (st != LRP_OK) return st;
  {
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    if (g_pool.size() <= (size_t)device) g_pool.resize((size_t)device + 1);
    auto &idle = g_pool[(size_t)device];
    if (!idle.empty()) {
      *out = idle.back();
      idle.pop_back();
      return LRP_OK;
    }
  }
  return lrp_context_create(out, device, 1);
}

void return_context(lrp_context *c) {
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  g_pool[(size_t)c->device].push_back(c);
}
} // namespace

int lrp_reproject(const lrp_image *in, lrp_image *out, int num_samples, int interpolation, const float *rotation,
                  const lrp_post *post, int device) {
  int st = validate(in, out, interpolation, true, true);
  if (st != LRP_OK) return st;
  lrp_context *c = nullptr;
  st = borrow_context(device, &c);
  if (st != LRP_OK) return st;
  st = lrp_context_submit(c, in, out, num_samples, interpolation, rotation, post);
  const int st_wait = lrp_context_wait(c);
  return_context(c);
  return st != LRP_OK ? st : st_wait;
}

int lrp_post_process(lrp_image *img, float exposure, float reinhard, int device) {
  if (!img || !img->data) return fail(LRP_ERR_NULL, "null image");
  if (img->width < 1 || img->height < 1 || img->channels < 1) return fail(LRP_ERR_BAD_DIMS, "bad image dimensions");
  if (!image_addressable(*img)) return fail(LRP_ERR_BAD_DIMS, "image too large (more than 2^31 floats)");
  lrp_context *c = nullptr;
  int st = borrow_context(device, &c);
  if (st != LRP_OK) return st;
  st = [&]() -> int {
    Slot &s = c->slots[0];
    const size_t bytes = image_bytes(*img);
    int r = s.d_out.reserve(bytes);
    if (r != LRP_OK) return r;
    LRP_HIP_TRY(hipMemcpyAsync(s.d_out.ptr, img->data, bytes, hipMemcpyHostToDevice, c->run));
    lrp_image d = *img;
    d.data = (float *)s.d_out.ptr;
    r = lrp_post_process_device(&d, exposure, reinhard, device, c->run);
    if (r != LRP_OK) return r;
    LRP_HIP_TRY(hipMemcpyAsync(img->data, s.d_out.ptr, bytes, hipMemcpyDeviceToHost, c->run));
    LRP_HIP_TRY(hipStreamSynchronize(c->run));
    return LRP_OK;
  }();
  return_context(c);
  return st;
}

int lrp_decode_pixels_device(const void *src, int src_format, int src_channels, float *dst, int dst_channels, size_t n_pixels,
                             int device, void *stream) {
  if (!src || !dst) return fail(LRP_ERR_NULL, "null buffer");
  if (!format_ok(src_format) || src_channels < 1 || dst_channels < 1 || src_channels > 64 || dst_channels > 64)
    return fail(LRP_ERR_BAD_ARG, "bad pixel format or channel count");
  int st = select_device(device);
  if (st != LRP_OK) return st;
  if (n_pixels == 0) return LRP_OK;
  hipError_t e = lrp::launch_decode_pixels(src, src_format, src_channels, dst, dst_channels, n_pixels, device, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "pixel decode kernel launch");
  return LRP_OK;
}

int lrp_encode_pixels_device(const float *src, int src_channels, void *dst, int dst_format, int dst_channels, unsigned fill,
                             size_t n_pixels, int device, void *stream) {
  if (!src || !dst) return fail(LRP_ERR_NULL, "null buffer");
  if (!format_ok(dst_format) || src_channels < 1 || dst_channels < 1 || src_channels > 64 || dst_channels > 64)
    return fail(LRP_ERR_BAD_ARG, "bad pixel format or channel count");
  int st = select_device(device);
  if (st != LRP_OK) return st;
  if (n_pixels == 0) return LRP_OK;
  hipError_t e = lrp::launch_encode_pixels(src, src_channels, dst, dst_format, dst_channels, fill, n_pixels, device, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "pixel encode kernel launch");
  return LRP_OK;
}

void lrp_pixel_tables(float decode[256], float threshold[256]) { lrp::pixel_tables_host(decode, threshold); }

int lrp_host_alloc(void **ptr, size_t bytes) {
  if (!ptr) return fail(LRP_ERR_NULL, "null pointer");
  *ptr = nullptr;
  if (device_count_cached() == 0) return fail(LRP_ERR_NO_DEVICE, "no HIP device visible");
  hipError_t e = hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault);
  if (e != hipSuccess) return hip_fail(e, "hipHostMalloc");
  return LRP_OK;
}

void lrp_host_free(void *ptr) {
  if (ptr) (void)hipHostFree(ptr);
}

int lrp_synth_fill_device(float *data, int width, int height, int channels, uint32_t seed, int depth_channel,
                          int device, void *stream) {
  if (!data) return fail(LRP_ERR_NULL, "null data");
  if (width < 1 || height < 1 || channels < 1) return fail(LRP_ERR_BAD_DIMS, "bad image dimensions");
  const unsigned long long n = (unsigned long long)width * height * channels;
  if (n > kMaxImageFloats) return fail(LRP_ERR_BAD_DIMS, "image too large (more than 2^31 floats)");
  int st = select_device(device);
  if (st != LRP_OK) return st;
  hipError_t e = lrp::launch_synth_fill(data, (uint32_t)n, channels, seed, depth_channel, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "synth_fill kernel launch");
  return LRP_OK;
}

int lrp_checksum_device(const float *data, size_t n, uint64_t *out, int device, void *stream) {
  if (!data || !out) return fail(LRP_ERR_NULL, "null array");
  if (n >= (1ull << 32)) return fail(LRP_ERR_BAD_DIMS, "buffer too large");
  int st = select_device(device);
  if (st != LRP_OK) return st;
  hipError_t e = lrp::launch_checksum(data, n, reinterpret_cast<unsigned long long *>(out), (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "checksum kernel launch");
  return LRP_OK;
}

int lrp_math_eval_device(int func, const float *a, const float *b, float *out, size_t n, int device, void *stream) {
  if (!a || !out) return fail(LRP_ERR_NULL, "null array");
  if (func < 0 || func > 9) return fail(LRP_ERR_BAD_ARG, "unknown function id");
  int st = select_device(device);
  if (st != LRP_OK) return st;
  if (n == 0) return LRP_OK;
  hipError_t e = lrp::launch_math_eval(func, a, b, out, n, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "math_eval kernel launch");
  return LRP_OK;
}

} // extern "C"
