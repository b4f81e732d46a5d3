/*
 * lrp.h — C ABI of the MI355X-native lens reprojection library (liblrp_hip.so).
 *
 * This is the drop-in boundary for the reference's L4 -> L1 call: the worker
 * lambda in reference src/main.cpp:597-603 calls
 *     reproject::reproject(&input, &output, num_samples, interpolation, rotation_matrix);
 *     reproject::post_process(&output, exposure, reinhard);
 * declared in reference src/reproject.hpp:22-27.  The reference has no FFI layer
 * of its own; a maintainer binds these entry points from the C++
 * wrapper in include/lens_reproject.hpp.
 *
 * Plain C: pointers, sizes, fixed-width enums.  No torch / HIP types appear in
 * the signatures (a HIP stream travels as void*).  Every function returns an
 * lrp_status; nothing exits the process or throws.  The library never falls
 * back to a CPU path: without a usable gfx950 device every compute entry point
 * fails with LRP_ERR_NO_DEVICE / LRP_ERR_HIP.
 *
 * Thread safety: all entry points may be called concurrently from different
 * host threads (the reference calls reproject() from -j N pool threads,
 * src/main.cpp:538-544).  An lrp_context must be used by one thread at a time.
 */
#ifndef LRP_H
#define LRP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRP_ABI_VERSION 3

/* ---- enums: numbering identical to the reference's ------------------------ */

/* reference src/config.hpp:7-13 (enum LensType) */
typedef enum lrp_lens_type {
  LRP_RECTILINEAR = 0,
  LRP_FISHEYE_EQUIDISTANT = 1,
  LRP_FISHEYE_EQUISOLID = 2,     /* declared by the reference, rejected by reproject(); rendered here once
                                    lrp_lens_extensions(LRP_LENS_EXT_EQUISOLID) is set */
  LRP_FISHEYE_STEREOGRAPHIC = 3, /* declared by the reference, rejected by reproject(); rendered here once
                                    lrp_lens_extensions(LRP_LENS_EXT_STEREOGRAPHIC) is set */
  LRP_EQUIRECTANGULAR = 4
} lrp_lens_type;

/* Opt-in lens extensions (lrp_lens_extensions).  LRP_LENS_EXT_EQUISOLID: LRP_FISHEYE_EQUISOLID, which the reference
 * declares and rejects, renders on either side.  This project defines its mapping (Blender's equisolid fisheye,
 * r = 2 f sin(theta / 2)) in binary32, un-fused, associated left to right, with cx, cy the centred sub-sample coordinates:
 *   equisolid_to_vec:  r_px = sqrtf(cx*cx + cy*cy); r_mm = r_px / img_w * sensor_width;
 *                      theta = 2.0f * asinf(r_mm / (2.0f * focal_length)); s = sinf(theta) / r_px;
 *                      x = s * cx; y = s * cy; z = cosf(theta)
 *   vec_to_equisolid:  x = x / -z; y = y / -z; r = sqrtf(x*x + y*y); theta = atanf(r);
 *                      r_mm = (2.0f * focal_length) * sinf(0.5f * theta); r_px = r_mm / sensor_width * img_w;
 *                      cx = x / r * r_px; cy = y / r * r_px
 * fov and sensor_height do not enter the mapping (in Blender fov only crops the image circle; nothing is masked, as for
 * every lens of the reference).  The centre pixel of an odd-sized output (r_px == 0) and the pixels beyond the image
 * circle (r_mm > 2f: asinf gives NaN) have NaN rays and render what the samplers make of NaN coordinates, like the
 * centre of an equidistant output.  Rays behind the camera fold through x / -z, as for the equidistant source. */
#define LRP_LENS_EXT_EQUISOLID 1
/* LRP_LENS_EXT_STEREOGRAPHIC: LRP_FISHEYE_STEREOGRAPHIC, likewise declared and rejected by the reference, renders on either
 * side.  The reference has no stereographic code; this project defines the mapping: the conformal fisheye (the "little planet"
 * projection of a panorama), r = 2 f tan(theta / 2).  It follows the equidistant and equisolid lenses in everything but the
 * radial law — image-circle scale by sensor_width / img_w only, target rays with z = cos(theta), source rays folded through
 * x / -z (the front hemisphere), sensor_height not used — and needs no libm call.  Binary32, un-fused, associated left to
 * right, F = 2.0f * focal_length (exact):
 *   stereographic_to_vec:  r_px = sqrtf(cx*cx + cy*cy); r_mm = r_px / img_w * sensor_width;
 *                          t = r_mm / F; t2 = t*t; d = 1.0f + t2;
 *                          s = ((2.0f * t) / d) / r_px;               (sin(theta) / r_px)
 *                          x = s * cx; y = s * cy; z = (1.0f - t2) / d   (cos(theta))
 *   vec_to_stereographic:  x = x / -z; y = y / -z; r = sqrtf(x*x + y*y);
 *                          t = r / (1.0f + sqrtf(1.0f + r*r));        (tan(atan(r) / 2))
 *                          r_mm = F * t; r_px = r_mm / sensor_width * img_w;
 *                          cx = x / r * r_px; cy = y / r * r_px
 * The radius is finite for every theta < pi: there is no "beyond the image circle", every pixel has a finite ray (a full
 * equirectangular panorama fits into one stereographic frame).  The centre pixel of an odd-sized output (r_px == 0) has a
 * NaN ray, like the equidistant centre.  The lens has one parameter, focal_length.
 * The value is 0x100: the low byte of the mask is spoken for (a mask of 0xFF reads back as LRP_LENS_EXT_EQUISOLID).  A
 * reprojection between an equisolid and a stereographic lens needs both bits. */
#define LRP_LENS_EXT_STEREOGRAPHIC 0x100

/* reference src/reproject.hpp:16-20 (enum Interpolation) */
typedef enum lrp_interpolation { LRP_NEAREST = 0, LRP_BILINEAR = 1, LRP_BICUBIC = 2 } lrp_interpolation;
/* Lanczos-3: an interpolation value outside the reference's enum (which keeps its three members), accepted only while
 * lrp_sampler_extensions(LRP_SAMPLER_EXT_LANCZOS3) is set; see "Lanczos-3" below. */
#define LRP_LANCZOS3 3
#define LRP_SAMPLER_EXT_LANCZOS3 1

/* reference src/reproject.hpp:7 (enum DataLayout); carried, never read by the kernels */
typedef enum lrp_data_layout { LRP_RGB = 0, LRP_RGBA = 1, LRP_RGBZ = 2, LRP_RGBAZ = 3 } lrp_data_layout;

typedef enum lrp_status {
  LRP_OK = 0,
  LRP_ERR_OUTPUT_LENS = 1,   /* reference prints "Output lens type not supported." and exit(1), src/reproject.cpp:415-417 */
  LRP_ERR_INPUT_LENS = 2,    /* "Input lens type not supported.",  src/reproject.cpp:395-397 */
  LRP_ERR_INTERPOLATION = 3, /* "Interpolation method not supported.", src/reproject.cpp:364-366 */
  LRP_ERR_CHANNELS = 4,      /* in->channels != out->channels (unchecked precondition in the reference) or < 1 */
  LRP_ERR_BAD_DIMS = 5,      /* non-positive size, or an image of more than 2^31 floats (what the reference's int indexing addresses) */
  LRP_ERR_NULL = 6,          /* NULL image / data pointer */
  LRP_ERR_NO_DEVICE = 7,     /* no HIP device, or device index out of range */
  LRP_ERR_HIP = 8,           /* a HIP runtime call failed; see lrp_last_error() */
  LRP_ERR_OOM = 9,           /* device or pinned-host allocation failed */
  LRP_ERR_BAD_ARG = 10
} lrp_status;

/* ---- PODs: layout identical to the reference's ----------------------------- */

/* reference src/config.hpp:15-37 (struct LensInfo): sizeof 28; type @0, union @4,
 * sensor_width @20, sensor_height @24.  Millimetres and radians. */
typedef struct lrp_lens {
  int32_t type; /* lrp_lens_type */
  union {
    struct { float focal_length; } rectilinear;
    struct { float fov; } fisheye_equidistant;
    struct { float focal_length; float fov; } fisheye_equisolid;
    struct { float focal_length; } fisheye_stereographic;
    struct { float latitude_min, latitude_max, longitude_min, longitude_max; } equirectangular;
    float raw[4];
  } u;
  float sensor_width;
  float sensor_height;
} lrp_lens;

/* reference src/reproject.hpp:9-14 (struct Image): sizeof 56; lens @0, width @28,
 * height @32, channels @36, data @40, data_layout @48.  Interleaved row-major
 * float32, data[(y*width + x)*channels + c], no row padding. */
typedef struct lrp_image {
  lrp_lens lens;
  int32_t width, height, channels;
  float *data;
  int32_t data_layout; /* lrp_data_layout */
} lrp_image;

/* Optional fused epilogue == reference post_process(img, exposure, reinhard)
 * (src/reproject.cpp:421-437) applied to the freshly written output.  The
 * reference CLI runs it when exposure != 1 || reinhard != 1 (src/main.cpp:601). */
typedef struct lrp_post {
  float exposure;
  float reinhard;
} lrp_post;

/* ---- library / device ------------------------------------------------------ */

int lrp_abi_version(void);
/* Process-wide mask of opt-in lens extensions (LRP_LENS_EXT_*), 0 by default: every entry point then rejects the lenses
 * the reference rejects, with its messages.  Sets the mask for subsequent calls of all threads (each call reads it once)
 * and returns the previous one; a negative value only queries.  The known bits (LRP_LENS_EXT_EQUISOLID,
 * LRP_LENS_EXT_STEREOGRAPHIC) are kept, the rest dropped.  With both on, every value of lrp_lens_type renders. */
int lrp_lens_extensions(int mask);
/* Process-wide mask of opt-in sampler extensions (LRP_SAMPLER_EXT_*), 0 by default: every entry point then rejects
 * interpolation 3 as the reference does, with LRP_ERR_INTERPOLATION.  The semantics of lrp_lens_extensions: sets the mask for
 * subsequent calls of all threads (each call reads it once) and returns the previous one; a negative value only queries; the
 * known bit (LRP_SAMPLER_EXT_LANCZOS3) is kept, the rest dropped. */
int lrp_sampler_extensions(int mask);
/* Number of usable HIP devices (0 when there is none; never negative). */
int lrp_device_count(void);
/* Static text for a status code. */
const char *lrp_strerror(int status);
/* Detail of the calling thread's last failure (HIP error string etc.), "" if none. */
const char *lrp_last_error(void);

/* Three HIP kernel families compute the same bits: 0 = one pixel per lane
 * (any channel count), 1 = tile kernel (RGB / RGBA / RGBAZ), 2 = tile kernel + LDS-window
 * bicubic (default; the library picks the pixel kernel by itself where the others
 * do not apply), 3 = as 2 with the window kernel's shared-coefficient tier switched off.  Testing / A-B knob: sets the family for subsequent calls of all
 * threads and returns the previous one; an out-of-range value only queries.  (The library reads no environment variable.) */
int lrp_debug_kernel(int choice);
/* The other testing / A-B switches, by name: "kernel" (as lrp_debug_kernel), "xsep", "quad", "mirror_modes",
 * "win_edge", "win_split", "geo_cache" (0 / 1: a sharing or staging path of the tile / window kernels off / on — the bits
 * do not change), "batch_frames" (frames per wavefront of a batched launch, 0 = automatic),
 * "multi_fork" (side streams of lrp_reproject_multi_device, 0-5), "geo_strip" (blocks per wavefront of a launch that reads the
 * geometry cache, 0 = automatic), "geo_big" (the big-window variant of those kernels: 1 = a rectilinear view rendered into a panorama and every geometry whose census says that
 * 30 % of its in-view blocks are too large for a 10 KiB window, 0 = never, 2 = always),
 * "geo_lists" (rendering by block class from the lists of a geometry-cache entry: 0 never, 1 where corner blocks are at least
 * 30 % of the frame, 2 whenever the lists are known), "geo_fill_fused" (0: the corner runs of such a launch always by the fill kernel, not as a share per
 * wavefront of the window kernel), "geo_fill_stream" (1: that fill kernel on a side stream), "big_launches" (a counter), "context_streams" (0: an lrp_context keeps all its kernels on one compute stream instead of alternating two),
 * "win_ss" (0: bicubic with num_samples 2-4 through the tile kernel instead of the window kernel's supersampling instantiations),
 * "geo_census" (0: no census of a new entry's windows), "geo_list_recs" (0: listed wavefronts read their block's record from the box array),
 * "win_tapdma" (0: passes of the big-window variant whose window fits no buffer gather per lane instead of fetching their taps quad by quad through LDS-DMA),
 * "listed_launches" (a counter: launches rendered by block class so far; 0 resets).  Sets the value for subsequent calls of all threads
 * and returns the previous one; a value outside the switch's range only queries; an unknown name returns -1. */
int lrp_debug_set(const char *name, int value);
/* Frees the cached per-output-lens tables and the geometry cache of every device (after
 * synchronising them).  Optional: both caches are bounded and reused across calls. */
void lrp_release_cached_tables(void);

/* ---- geometry cache ---------------------------------------------------------- */

/* The reference renders a whole run with ONE geometry — lenses, sizes and rotation are command-line
 * constants, only the pixels change from file to file (src/main.cpp:576-598) — and derives the source
 * coordinates of every output pixel again for every file (src/reproject.cpp:287-324).  Here the first
 * single-image bicubic launch of a geometry (lrp_reproject, lrp_reproject_device,
 * lrp_reproject_multi_device, lrp_context_submit*) leaves those coordinates in device memory as a side
 * output (8 bytes per output pixel + 2 per 16 pixels) and later launches of the same geometry on that device load them
 * instead of computing them: same values, same rendered bits, 1.2-1.9x the kernel rate.  Keyed on
 * (device, both lenses, both sizes, rotation, num_samples); least recently used entries are dropped when
 * `max_bytes` per device would be exceeded; a launch being captured into a hipGraph does not use it.
 * num_samples 2-4 (the reference's --samples) keep an entry of their own kind, shared by the three samplers: a coordinate
 * pair per SUB-SAMPLE, 8 x num_samples^2 bytes per output pixel.
 *   max_bytes      bytes per device (default: min(4 GiB, 2 % of the device's memory), at least two entries of the largest
 *                  geometry seen; -2 restores it); 0 switches the cache off and frees it; -1 keeps the value
 *   min_sightings  a geometry is cached from its n-th launch on (default 1; 2 suits callers whose
 *                  rotation changes with every call — the library switches to 2 by itself after
 *                  evicting several entries that were never read); < 1 keeps the value */
int lrp_geometry_cache_configure(long long max_bytes, int min_sightings);
typedef struct lrp_geometry_cache_info {
  uint64_t bytes, max_bytes, entries; /* device memory held now (all devices), the per-device limit, geometries held */
  uint64_t fills, hits, bypasses, evictions; /* launches that wrote an entry / read one / ran without the cache; entries dropped */
} lrp_geometry_cache_info;
void lrp_geometry_cache_stats(lrp_geometry_cache_info *out);

/* ---- one image, host buffers (the reference's calling convention) ---------- */

/* Drop-in for reproject::reproject (src/reproject.cpp:405-419) with in->data and
 * out->data in host memory (pageable or pinned).  Uploads the source, runs the
 * kernel on `device`, downloads the result; returns when out->data is complete.
 * rotation: 9 floats row-major or NULL (= no rotation, src/reproject.cpp:303).
 * post: NULL, or the fused post_process epilogue.
 * num_samples <= 0 leaves out->data untouched, as the reference loop does. */
int lrp_reproject(const lrp_image *in, lrp_image *out, int num_samples, int interpolation,
                  const float *rotation, const lrp_post *post, int device);

/* Drop-in for reproject::post_process (src/reproject.cpp:421-437), host buffer. */
int lrp_post_process(lrp_image *img, float exposure, float reinhard, int device);

/* ---- one image, device-resident buffers ------------------------------------ */

/* Same operation with in->data / out->data being device pointers on `device`.
 * Asynchronous: enqueues on `stream` (a hipStream_t, NULL = default stream) and
 * returns; the caller synchronises.  The first call with a new (output lens,
 * output size, num_samples) builds that lens's per-column / per-row tables
 * (one small allocation + a synchronous 2-microsecond kernel, cached afterwards);
 * every later call neither allocates nor synchronises and is capturable into a
 * hipGraph. */
int lrp_reproject_device(const lrp_image *in, lrp_image *out, int num_samples, int interpolation,
                         const float *rotation, const lrp_post *post, int device, void *stream);

int lrp_post_process_device(lrp_image *img, float exposure, float reinhard, int device, void *stream);

/* One resident source, n_out target lenses/rotations (cubemap faces etc.):
 * outs[i] is rendered with rotations + 9*i (or no rotation when rotations is
 * NULL).  Equivalent to n_out reference calls sharing `in`. */
int lrp_reproject_multi_device(const lrp_image *in, lrp_image *outs, int n_out, int num_samples,
                               int interpolation, const float *rotations, const lrp_post *post,
                               int device, void *stream);

/* Rows [row_first, row_first + row_count) of the output only (out->data is the whole image; the rows
 * of the reference loop are independent, src/reproject.cpp:284): what a job that splits one output over
 * several GPUs or streams launches.  The bytes are those of the same rows of a whole-image call. */
int lrp_reproject_rows_device(const lrp_image *in, lrp_image *out, int num_samples, int interpolation,
                              const float *rotation, const lrp_post *post, int row_first, int row_count,
                              int device, void *stream);

/* n images of ONE geometry (same sizes, channel count, lenses; one rotation, one
 * post setting — a directory of frames from one camera, src/main.cpp:540-622) on
 * device-resident buffers: rendered by one kernel launch per 16 images instead of
 * one per image, so the GPU does not drain and refill between frames.  Results are
 * those of n lrp_reproject_device calls. */
int lrp_reproject_batch_device(const lrp_image *ins, lrp_image *outs, int n, int num_samples,
                               int interpolation, const float *rotation, const lrp_post *post,
                               int device, void *stream);

/* ---- coverage planes: which output pixels the source can see ------------------------ */

/* The render entry points reproduce what the reference does with a ray the source image never recorded: its samplers clamp,
 * so a coordinate outside the source smears the border texel (src/reproject.cpp:45-47,63-67,119-127), and the sources that
 * fold a ray through x / -z (rectilinear :163-164, equidistant :191-192, and the two extension lenses above) render a
 * mirrored ghost of the picture for a ray behind the camera.  The coverage of a call says which output pixels are real.
 *
 * Definition, for output pixel (x, y) and sub-sample (ssx, ssy) of a num_samples = n call: vx, vy, vz is the ray after the
 * optional rotation (src/reproject.cpp:301-311), sx, sy the top-left-origin coordinates the sampler receives (:323-324) —
 * binary32, un-fused, exactly the values the render kernels compute.  The sub-sample is COVERED iff
 *   front:  vz < 0.0f for a source that folds through x / -z (rectilinear, equidistant, equisolid, stereographic); always
 *           true for an equirectangular source;
 *   in_x:   sx == sx for a wrapping source (LoopHorizontally, :386-390); sx >= -0.5f && sx <= (float)in_w - 0.5f otherwise;
 *   in_y:   sy >= -0.5f && sy <= (float)in_h - 0.5f
 * all hold.  Comparisons with NaN are false: a NaN ray (the centre of an odd-sized fisheye output, the area beyond the
 * equisolid image circle) is uncovered.  The COVERAGE COUNT of a pixel is the number of its covered sub-samples, 0 .. n * n,
 * one uint8_t per output pixel; the plane is row-major without padding.
 *
 * lrp_coverage_device: asynchronous on `stream`; neither allocates nor synchronises.  in->data is never read and may be NULL
 * (in->channels is not looked at).  Whatever is requested is done by one kernel launch:
 *   coverage        device pointer of any alignment, or NULL: receives the count plane (out->width * out->height bytes);
 *   mask_image != 0 every channel of every pixel of out->data (a device pointer) whose count is 0 becomes +0.0f; every other
 *                   pixel keeps its bytes;
 *   alpha_channel   in [0, out->channels): that channel of EVERY pixel of out->data becomes (float)count * (1.0f / (float)(n * n))
 *                   (the reference's normalize, :280), applied after the mask; -1: off.
 * Errors: the lens, extension-mask and size errors of lrp_reproject_device, in its order and with its statuses (an equisolid
 * or stereographic lens needs its extension bit; the interpolation check has no counterpart); then LRP_ERR_BAD_ARG for nothing
 * requested (coverage == NULL, no mask, no alpha), num_samples < 1 or > 15, or an alpha_channel outside [-1, out->channels);
 * LRP_ERR_CHANNELS / LRP_ERR_NULL for a mask or alpha request with out->channels < 1 / out->data == NULL.  The geometry cache
 * is neither read nor written: the lrp_geometry_cache_stats counters do not move. */
int lrp_coverage_device(const lrp_image *in, const lrp_image *out, int num_samples, const float *rotation,
                        uint8_t *coverage, int mask_image, int alpha_channel, int device, void *stream);

/* ---- compose: several source images into one output ------------------------------------ */

/* The opposite direction of lrp_reproject_multi_device: n_in device-resident sources (six cube faces, the two fisheyes of a
 * 360-degree camera, a rig of overlapping cameras), each with its own lens parameters, size and rotation, rendered into ONE
 * output by one kernel launch (per group of 8 channels).  Per output pixel the target ray is computed once, each source is
 * asked in turn whether it recorded that ray — the coverage definition above — and only the sources that did are sampled.
 *
 * Definition.  num_samples is 1 (lrp_compose_ss_device below takes num_samples).  All arithmetic is binary32, un-fused, in the order written; min(a, b) is (b < a) ? b : a.
 * For output pixel (x, y) and source i: vx, vy, vz is the pixel's target ray after rotation i (rotations + 9 * i; the rotation
 * and the operations of lrp_reproject_device(ins + i, out, 1, ..., rotations + 9 * i); rotations == NULL: no source is rotated,
 * no multiplication happens), sx, sy the coordinates that source's sampler would receive.  Source i COVERS the pixel iff that
 * sub-sample is covered under the coverage definition above (front && in_x && in_y, comparisons with NaN false).
 * s_i is the texel sample<interpolation> returns for (sx, sy) in source i: bit for bit what lrp_reproject_device stores for the
 * pixel before any post.  k is the number of covering sources.
 *   LRP_COMPOSE_FIRST    the pixel is s_i of the lowest-numbered covering source;
 *   LRP_COMPOSE_MEAN     acc_c = +0.0f; for ascending covering i: acc_c = acc_c + s_i,c; the pixel is acc_c / (float)k;
 *   LRP_COMPOSE_FEATHER  dy = min(sy + 0.5f, ((float)in_h - 0.5f) - sy); dx likewise from sx and in_w (the distance, in texels, to
 *                        the nearer edge of source i); m = dy for a wrapping equirectangular source, else m = min(dx, dy);
 *                        w_i = (m < 0x1p-10f) ? 0x1p-10f : m; acc_c = +0.0f, W = +0.0f; for ascending covering i:
 *                        acc_c = acc_c + w_i * s_i,c (multiply, then add), W = W + w_i; the pixel is acc_c / W.
 * A pixel no source covers (k == 0) becomes +0.0f in every channel.  post: the reference's tonemap on the first min(C, 3)
 * channels of the composed value, as in every other entry point; a k == 0 pixel stays +0.0f in every channel whatever post is.
 * count: a device pointer of any alignment, or NULL: receives k per pixel, out->width * out->height bytes, row-major, unpadded.
 *
 * Asynchronous on `stream`; allocates nothing, does not synchronise, builds no lens table, neither reads nor writes the geometry
 * cache (the lrp_geometry_cache_stats counters do not move).
 * Errors, all before a device is touched, in this order: n_in outside 1 .. LRP_COMPOSE_MAX_SOURCES or an unknown mode:
 * LRP_ERR_BAD_ARG; ins or out NULL: LRP_ERR_NULL; per source, in ascending order, the checks of lrp_reproject_device(ins + i, out)
 * with its statuses (lens and extension bits, interpolation, channels — every source has out->channels channels, else
 * LRP_ERR_CHANNELS —, sizes, data pointers); then all sources must resolve to the same source mode — rectilinear, equidistant,
 * clamped equirectangular, wrapping equirectangular (a full turn of longitude), equisolid, stereographic —, else LRP_ERR_BAD_ARG
 * with an lrp_last_error text that names the two modes.  Sizes, lens parameters and rotations may differ per source. */
#define LRP_COMPOSE_MAX_SOURCES 8
typedef enum lrp_compose_mode { LRP_COMPOSE_FIRST = 0, LRP_COMPOSE_MEAN = 1, LRP_COMPOSE_FEATHER = 2 } lrp_compose_mode;
int lrp_compose_device(const lrp_image *ins, int n_in, const float *rotations /* n_in x 9, or NULL */, const lrp_image *out,
                       int interpolation, int mode, const lrp_post *post, uint8_t *count /* out->width * out->height bytes, or NULL */,
                       int device, void *stream);

/* ---- compose, supersampled: anti-aliased stitching in one launch ------------------------ */

/* lrp_compose_device with num_samples: several large frames composed into a smaller panorama (the reference's --scale 0.5
 * --samples 2 job, and likewise 3 and 4), one kernel launch per group of 8 channels.  Which sources cover a point is decided
 * per sub-sample, not per pixel.
 *
 * Definition.  All arithmetic is binary32, un-fused, in the order written.  n = num_samples, 1 .. 15.
 * Sub-sample (ssx, ssy), 0 <= ssx, ssy < n, of output pixel (x, y) sits where an n-sample lrp_reproject_device /
 * lrp_coverage_device call puts it: scx = cx + ((float)ssx + 1.0f) / ((float)n + 1.0f) - 0.5f with cx the pixel centre in
 * image-centred coordinates (src/reproject.cpp:287-298), scy likewise.  Sub-samples are numbered j = ssx * n + ssy (ssx the
 * outer loop, ssy the inner: the reference's loop order).  For sub-sample j: the target ray; per source i rotation i, sx, sy,
 * covered / not covered by the coverage definition, s_i and (FEATHER) w_i — all exactly as the compose definition above does
 * for its single sub-sample.  k_j is the number of sources that cover sub-sample j; v_j its composed value under `mode`
 * (FIRST / MEAN / FEATHER as defined for lrp_compose_device), +0.0f in every channel when k_j == 0.  m is the number of
 * sub-samples with k_j >= 1.  acc_c = +0.0f; for ascending j with k_j >= 1: acc_c = acc_c + v_j,c.  m == 0: the pixel is +0.0f
 * in every channel, whatever post is.  Otherwise r = 1.0f / (float)m and the pixel is acc_c * r (with m == n * n the
 * reference's normalize multiply, :280,338-341), then post on the first min(C, 3) channels.  Dividing by the covered sub-samples
 * rather than by n * n keeps edges and seams from fading to black; a caller who wants premultiplied edges multiplies by
 * coverage / (n * n).
 *   count     device pointer of any alignment, or NULL: per pixel the number of sources that cover at least one of its sub-samples;
 *   coverage  device pointer of any alignment, or NULL: per pixel m, 0 .. n * n.
 * Both planes are out->width * out->height bytes, row-major, unpadded.  With more than 8 channels there is one launch per group
 * of 8, and each writes the planes, with the same bytes.
 *
 * Relations:
 *   n == 1: the bytes of lrp_compose_device, except that a -0.0f channel becomes +0.0f (the accumulation starts from +0.0f);
 *           count is equal; coverage is k > 0.
 *   One source, FIRST or MEAN, a pixel with m == n * n: bit for bit what lrp_reproject_device(ins, out, n, interpolation,
 *           rotation) stores.
 *
 * Asynchronous on `stream`; allocates nothing, does not synchronise, builds no lens table, neither reads nor writes the geometry
 * cache.  Errors, all before a device is touched: those of lrp_compose_device in its order (interpolation 0 .. 2 only, one source
 * mode for all sources), then LRP_ERR_BAD_ARG for num_samples < 1 or > 15. */
int lrp_compose_ss_device(const lrp_image *ins, int n_in, const float *rotations /* n_in x 9, or NULL */, const lrp_image *out,
                          int num_samples, int interpolation, int mode, const lrp_post *post,
                          uint8_t *count /* out->width * out->height bytes, or NULL */,
                          uint8_t *coverage /* out->width * out->height bytes, or NULL */, int device, void *stream);

/* ---- compose, calibrated cameras: Brown-Conrady and fisheye polynomials ------------------ */

/* lrp_compose_ss_device for the frames of real cameras.  The sources of the two compose calls above are ideal lenses: the
 * optical axis in the centre of the frame, one focal length, no distortion.  A calibration delivers fx, fy, cx, cy in pixels
 * and distortion coefficients; both common models are closed-form polynomials in the direction this library needs — from ray
 * to source pixel —, so a calibrated frame is composed as it is, without an undistorted copy.  Undistorting one image is the
 * n_in == 1 case: a calibrated source into a rectilinear target.
 *
 * Definition.  Everything is the definition of lrp_compose_ss_device — sub-sample positions and order, FIRST / MEAN / FEATHER,
 * m, the 1.0f / (float)m normalisation, post, both planes, one launch per group of 8 channels — with two things replaced, for
 * camera i and the ray vx, vy, vz after rotation i: the source coordinates sx, sy and the coverage test.  Binary32, un-fused,
 * in the order written; k1 .. are the camera's k[]:
 *   LRP_CAMERA_BROWN (Brown-Conrady, k = k1 k2 p1 p2 k3: OpenCV's order)
 *     a = vx / -vz;  b = vy / -vz;  r2 = a*a + b*b;  ab = a*b;
 *     L  = 1.0f + r2*(k1 + r2*(k2 + r2*k3));
 *     xd = a*L + ((2.0f*p1)*ab + p2*(r2 + 2.0f*(a*a)));
 *     yd = b*L + (p1*(r2 + 2.0f*(b*b)) + (2.0f*p2)*ab);
 *     sx = fx*xd + cx;  sy = fy*yd + cy;                      imaged = vz < 0.0f && r2 <= limit
 *   LRP_CAMERA_FISHEYE (Kannala-Brandt, k = k1 k2 k3 k4: the order of OpenCV's fisheye module; k[4] is ignored)
 *     rho = sqrtf(vx*vx + vy*vy);  theta = atan2f(rho, -vz);  t2 = theta*theta;
 *     td  = theta*(1.0f + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4))));
 *     q   = (rho > 0.0f) ? td / rho : 0.0f;
 *     sx  = fx*(q*vx) + cx;  sy = fy*(q*vy) + cy;             imaged = theta <= limit
 * A sub-sample is COVERED by camera i iff imaged && sx >= -0.5f && sx <= (float)width - 0.5f && sy >= -0.5f &&
 * sy <= (float)height - 0.5f, comparisons with NaN being false.  s_i is sample<interpolation> at (sx, sy), clamping and never
 * wrapping; FEATHER's dx, dy, w_i are those of the compose definition (m = min(dx, dy)).
 * Axes: the library's — x right, y down, the camera looks down -z; OpenCV's camera frame with z_cv = -vz.  (0, 0) is the
 * CENTRE of the top-left texel, as in the samplers' sx, sy and in OpenCV.  The fisheye takes the angle from atan2f, not from a
 * fold through x / -z: a camera that sees behind itself (190 - 220 degree lenses) is expressible, with limit up to pi.
 * limit exists because both polynomials stop being monotonic off axis: without it, rays far outside the field of view fold
 * back into the frame as ghosts.  +inf is allowed.  The models may be mixed in one call.
 *
 * lrp_camera_limit (host only, evaluated in double): BROWN: the r2 = r * r of the last r on an ascending scan for which
 * g(r) = r * L(r * r) still increases (the tangential terms do not enter); +inf when g increases up to r = 16.  FISHEYE: the
 * last theta for which td(theta) still increases; (float)pi when it does so up to pi.  The scan steps by 1 / 1024 (BROWN) or
 * pi / 4096 (FISHEYE); the step at which the function stops increasing brackets the turning point, and the bracket is then
 * bisected on the sign of the derivative, keeping the lower end where it is positive.  When a turning point t exists (for BROWN
 * t is the r2 at the turning point), the result v satisfies 0.99 * t <= v <= t; v is rounded down to float.  cam->data,
 * width, height, fx, fy, cx, cy and limit are not looked at.  Errors: cam or limit NULL: LRP_ERR_NULL; an unknown model or a
 * used coefficient that is not finite: LRP_ERR_BAD_ARG.
 *
 * lrp_compose_cameras_device: asynchronous on `stream`; allocates nothing, does not synchronise, builds no lens table, neither
 * reads nor writes the geometry cache (the lrp_geometry_cache_stats counters do not move).  Errors, all before a device is
 * touched, in this order:
 *   1. n_in outside 1 .. LRP_COMPOSE_MAX_SOURCES or an unknown mode: LRP_ERR_BAD_ARG;
 *   2. cams or out NULL: LRP_ERR_NULL;
 *   3. the output-side checks of lrp_compose_ss_device: the output lens and its extension bit (LRP_ERR_OUTPUT_LENS),
 *      out->channels < 1 (LRP_ERR_CHANNELS), a non-positive size or more than 2^31 floats (LRP_ERR_BAD_DIMS), out->data NULL
 *      (LRP_ERR_NULL);
 *   4. interpolation outside 0 .. 2: LRP_ERR_INTERPOLATION;
 *   5. per camera, ascending: an unknown model: LRP_ERR_BAD_ARG; a non-positive size or more than 2^31 floats
 *      (width * height * out->channels): LRP_ERR_BAD_DIMS; data NULL: LRP_ERR_NULL; fx, fy, cx, cy or a used k not finite, fx or
 *      fy equal to 0, or limit NaN or negative: LRP_ERR_BAD_ARG with an lrp_last_error text that names the camera index and the
 *      field ("camera 2: k[1] ...");
 *   6. num_samples outside 1 .. 15: LRP_ERR_BAD_ARG. */
typedef enum lrp_camera_model { LRP_CAMERA_BROWN = 0, LRP_CAMERA_FISHEYE = 1 } lrp_camera_model;
typedef struct lrp_camera {
  int32_t model;          /* lrp_camera_model */
  int32_t width, height;  /* the frame; it has out->channels channels */
  const float *data;      /* device pointer, interleaved float32 like lrp_image */
  float fx, fy, cx, cy;   /* pixels; (0, 0) is the CENTRE of the top-left texel */
  float k[5];             /* BROWN: k1 k2 p1 p2 k3.  FISHEYE: k1 k2 k3 k4, k[4] ignored */
  float limit;            /* BROWN: largest r2 that is imaged; FISHEYE: largest theta (radians).  +inf allowed */
} lrp_camera;
int lrp_compose_cameras_device(const lrp_camera *cams, int n_in, const float *rotations /* n_in x 9, or NULL */,
                               const lrp_image *out, int num_samples, int interpolation, int mode, const lrp_post *post,
                               uint8_t *count /* out->width * out->height bytes, or NULL */,
                               uint8_t *coverage /* out->width * out->height bytes, or NULL */, int device, void *stream);
int lrp_camera_limit(const lrp_camera *cam, float *limit);

/* ---- calibrated camera as the target: a new camera matrix, camera to camera, re-distortion ---- */

/* lrp_compose_cameras_device whose OUTPUT is the frame of a calibrated camera too: an undistorted or rectified view with its
 * own fx, fy, cx, cy (OpenCV's newCameraMatrix), the frame of camera A as camera B would have recorded it (Kannala-Brandt to
 * Brown-Conrady and back), a rendering with the distortion of a real lens.  The polynomials are closed-form from ray to pixel;
 * the target needs the other direction, pixel to ray, and gets it from a fixed number of Newton steps.
 *
 * Definition.  Everything is the definition of lrp_compose_cameras_device — the sources, rotations, coverage per sub-sample,
 * FIRST / MEAN / FEATHER, m, 1.0f / (float)m, post, both planes, one launch per group of 8 channels — with the target ray
 * replaced.  The target is an lrp_camera T: T.data is ignored, T.width and T.height are the output size.  For output pixel
 * x, y and sub-sample ssx, ssy (the order of lrp_compose_ss_device), n = num_samples, ns1 = (float)n + 1.0f; binary32,
 * un-fused, in the order written; k1 .. are T.k[]:
 *   u  = ((float)x + ((float)ssx + 1.0f) / ns1) - 0.5f;   v likewise from y, ssy          (n == 1: u == x exactly)
 *   x0 = (u - T.cx) / T.fx;   y0 = (v - T.cy) / T.fy;
 *   LRP_CAMERA_BROWN
 *     X = x0;  Y = y0;  ok = (X*X + Y*Y <= T.limit);
 *     repeat LRP_CAMERA_INVERSE_STEPS times:
 *       r2 = X*X + Y*Y;  ab = X*Y;
 *       L  = 1.0f + r2*(k1 + r2*(k2 + r2*k3));          D = k1 + r2*((2.0f*k2) + r2*(3.0f*k3));
 *       xd = X*L + ((2.0f*p1)*ab + p2*(r2 + 2.0f*(X*X)));   yd = Y*L + (p1*(r2 + 2.0f*(Y*Y)) + (2.0f*p2)*ab);
 *       ex = xd - x0;  ey = yd - y0;
 *       jxx = ((L + (2.0f*(X*X))*D) + (2.0f*p1)*Y) + (6.0f*p2)*X;
 *       jxy = (((2.0f*ab)*D) + (2.0f*p1)*X) + (2.0f*p2)*Y;
 *       jyy = ((L + (2.0f*(Y*Y))*D) + (6.0f*p1)*Y) + (2.0f*p2)*X;
 *       det = jxx*jyy - jxy*jxy;
 *       Xn = X - (jyy*ex - jxy*ey)/det;   Yn = Y - (jxx*ey - jxy*ex)/det;   X = Xn;  Y = Yn;
 *       ok = ok && (X*X + Y*Y <= T.limit);                    (a comparison with NaN is false, and ok stays false)
 *     once more r2, ab, L, xd, yd, ex, ey at the final X, Y;
 *     has_ray = ok && fabsf(T.fx*ex) <= 0.5f && fabsf(T.fy*ey) <= 0.5f;          ray = (X, Y, -1.0f)
 *   LRP_CAMERA_FISHEYE
 *     rd = sqrtf(x0*x0 + y0*y0);  th = rd;  ok = (th <= T.limit);
 *     repeat LRP_CAMERA_INVERSE_STEPS times:
 *       t2 = th*th;
 *       g  = th*(1.0f + t2*(k1 + t2*(k2 + t2*(k3 + t2*k4))));
 *       gp = 1.0f + t2*((3.0f*k1) + t2*((5.0f*k2) + t2*((7.0f*k3) + t2*(9.0f*k4))));
 *       th = th - (g - rd)/gp;     ok = ok && th >= 0.0f && th <= T.limit;
 *     once more t2, g at the final th;  e = g - rd;
 *     has_ray = ok && fabsf(T.fx*e) <= 0.5f && fabsf(T.fy*e) <= 0.5f;
 *     sincosf(th) -> s, c;  q = (rd > 0.0f) ? s/rd : 0.0f;                       ray = (q*x0, q*y0, -c)
 * A sub-sample without a ray is covered by no camera: it adds nothing and is counted neither in m nor in count nor in coverage.
 * A target frame that reaches beyond the point where its own polynomial turns has pixels without a ray; they are +0.0f with
 * coverage 0, not ghosts.  The BROWN ray is not normalised: both source mappings are invariant to the length of the ray.  ok is
 * sticky because an iterate that has left the region where the polynomial is monotonic may wander back in by accident.  Newton
 * with the full 2 x 2 Jacobian, not OpenCV's fixed-point iteration, which converges linearly, and near the turning point not at
 * all.  The residual test (half a pixel) rejects what 8 steps did not bring home.
 *
 * lrp_camera_view_device: asynchronous on `stream`; allocates nothing, does not synchronise, builds no table, neither reads nor
 * writes the geometry cache.  out_data: target->width * target->height * channels floats on the device; every camera has
 * `channels` channels.  count, coverage: target->width * target->height bytes each, or NULL.  Errors, all before a device is
 * touched, in this order:
 *   1. n_in outside 1 .. LRP_COMPOSE_MAX_SOURCES or an unknown mode: LRP_ERR_BAD_ARG;
 *   2. cams, target or out_data NULL: LRP_ERR_NULL;
 *   3. the target: an unknown model: LRP_ERR_BAD_ARG; a non-positive size or more than 2^31 floats (width * height * channels):
 *      LRP_ERR_BAD_DIMS; fx, fy, cx, cy or a used k not finite, fx or fy equal to 0, or limit NaN or negative: LRP_ERR_BAD_ARG
 *      with an lrp_last_error text that begins "target: ".  limit need not be finite: with +inf, ok rests on NaN alone;
 *   4. channels < 1: LRP_ERR_CHANNELS;
 *   5. interpolation outside 0 .. 2: LRP_ERR_INTERPOLATION;
 *   6. per camera, ascending: the checks of lrp_compose_cameras_device;
 *   7. num_samples outside 1 .. 15: LRP_ERR_BAD_ARG.
 *
 * lrp_camera_unproject (host only): the definition from x0, y0 on, for n given positions u, v in pixels: rays[3 * j ..] and
 * has_ray[j] (or NULL), the bits of the device.  It is the library's undistortPoints.  cam->data, width and height are not
 * looked at.  Errors: cam, uv or rays NULL: LRP_ERR_NULL; n < 0, an unknown model, or fx, fy, cx, cy, a used k or limit that
 * the target checks above refuse: LRP_ERR_BAD_ARG.
 *
 * An ideal pinhole or equidistant SOURCE is expressible as a camera with k = 0; an equirectangular one is not. */
#define LRP_CAMERA_INVERSE_STEPS 8
int lrp_camera_view_device(const lrp_camera *cams, int n_in, const float *rotations /* n_in x 9, or NULL */,
                           const lrp_camera *target, float *out_data, int channels, int num_samples, int interpolation,
                           int mode, const lrp_post *post, uint8_t *count /* target->width * target->height bytes, or NULL */,
                           uint8_t *coverage /* target->width * target->height bytes, or NULL */, int device, void *stream);
int lrp_camera_unproject(const lrp_camera *cam, const float *uv /* n x 2, pixels */, int n, float *rays /* n x 3 */,
                         uint8_t *has_ray /* n, or NULL */);

/* ---- exposure matching across a camera rig: overlap statistics, gains, compose with gains ---- */

/* Cameras on auto-exposure differ by a third of a stop or more; FIRST then shows a step at every seam, MEAN and FEATHER a band.
 * Three calls measure and remove it: the statistic of the pairwise overlaps in one launch, Brown and Lowe's gain compensation
 * on the host, and lrp_compose_cameras_device with one gain per camera.
 *
 * lrp_camera_overlap_device.  Definition, binary32, un-fused, in the order written.  For each output pixel take the single
 * sub-sample of num_samples == 1 (the pixel centre).  The target ray, rotation i, sx, sy, imaged and covered_i are exactly those
 * of lrp_compose_cameras_device.  C = out->channels (the frames' stride).  s_i is the BILINEAR sample of the first min(C, 3)
 * channels of camera i at (sx, sy); the sampler is fixed.
 *   Y_i     = s_i[0]                                                  when C < 3, otherwise
 *   Y_i     = (0.25f * s_i[0] + 0.5f * s_i[1]) + 0.25f * s_i[2];
 *   valid_i = covered_i && Y_i >= lo && Y_i <= hi                     (comparisons with NaN are false)
 *   q_i     = (uint32_t)(Y_i * 65536.0f)                              (0 <= lo <= hi <= 32768: exact, at most 2^31)
 * For all i, j < n_in, the diagonal included:
 *   stats[(i * 8 + j) * 2]     = N_ij, the number of pixels with valid_i && valid_j;
 *   stats[(i * 8 + j) * 2 + 1] = S_ij, the sum of q_i over those pixels.
 * Every other word is 0: the call overwrites all LRP_OVERLAP_WORDS words, whatever they held.  The zeroing runs on `stream` ahead
 * of the kernel; the host does not synchronise.  The sums are integers — the result does not depend on the order of addition and
 * is exact; with out->width * out->height <= 2^31, S_ij < 2^63.  lo, hi exclude clipped and near-black pixels.
 * Asynchronous on `stream`; allocates nothing, builds no table, neither reads nor writes the geometry cache.  out: lens and size
 * only; out->data is not looked at and may be NULL.  Errors, all before a device is touched: those of
 * lrp_compose_cameras_device, items 1 to 5, in their order, out->data exempt from the NULL check (the interpolation is fixed:
 * item 4 cannot occur); then stats NULL: LRP_ERR_NULL; then lo or hi not finite, or not 0 <= lo <= hi <= 32768: LRP_ERR_BAD_ARG.
 *
 * lrp_camera_gains (host only, double, pure).  Brown and Lowe's gain compensation, as in OpenCV's GainCompensator.  stats is a
 * HOST copy of the table.  With I_ij = S_ij / (65536.0 * N_ij), taken as 0 where N_ij == 0, it minimises
 *   e = 1/2 * sum_i sum_j N_ij * ((g_i I_ij - g_j I_ji)^2 / sigma_n^2 + (1 - g_i)^2 / sigma_g^2).
 * The active set is the cameras with N_kk > 0; a camera with N_kk == 0 gets gain 1.0f and leaves the system.  For the active set
 *   A[k][k] = sum_{j != k} 2 N_kj I_kj^2 / sigma_n^2 + sum_j N_kj / sigma_g^2        (the second sum includes j == k)
 *   A[k][j] = -2 N_kj I_kj I_jk / sigma_n^2
 *   b[k]    = sum_j N_kj / sigma_g^2
 * and A g = b is solved in double by Gaussian elimination with partial pivoting; gains[k] = (float)g_k.  The table is symmetric
 * in N by construction, and the function relies on that.  sigma_n is in units of Y; OpenCV's values are 10 / 255 and 0.1.
 * Errors: stats or gains NULL: LRP_ERR_NULL; n_in outside 1 .. 8: LRP_ERR_BAD_ARG; a sigma that is not finite or not positive:
 * LRP_ERR_BAD_ARG.
 *
 * lrp_compose_cameras_gain_device.  The definition of lrp_compose_cameras_device with one insertion: right after sampling,
 * s_i[c] = g_i * s_i[c] for the absolute channels c < min(C, 3), g_i = gains[i] — one multiplication per channel, before the
 * FIRST / MEAN / FEATHER arithmetic, so that FEATHER forms w_i * (g_i * s_i[c]).  Alpha, depth and every further channel are
 * untouched (with more than 8 channels only the first group's launch multiplies).  Coverage, both planes and post are unchanged.
 * gains is a HOST array of n_in floats.  Errors: those of lrp_compose_cameras_device in their order; gains NULL: LRP_ERR_NULL,
 * checked with item 2; a gain that is not finite or is negative: LRP_ERR_BAD_ARG with an lrp_last_error text that names the
 * camera ("camera 2: gain ..."), checked after item 5. */
#define LRP_OVERLAP_WORDS 128 /* 8 x 8 x 2 uint64_t, whatever n_in is */
int lrp_camera_overlap_device(const lrp_camera *cams, int n_in, const float *rotations /* n_in x 9, or NULL */,
                              const lrp_image *out /* lens and size only; data is not looked at, may be NULL */, float lo, float hi,
                              uint64_t *stats /* DEVICE, LRP_OVERLAP_WORDS words */, int device, void *stream);
int lrp_camera_gains(const uint64_t *stats /* HOST copy */, int n_in, float sigma_n, float sigma_g, float *gains /* n_in */);
int lrp_compose_cameras_gain_device(const lrp_camera *cams, int n_in, const float *rotations /* n_in x 9, or NULL */,
                                    const float *gains /* HOST, n_in */, const lrp_image *out, int num_samples, int interpolation,
                                    int mode, const lrp_post *post, uint8_t *count /* out->width * out->height bytes, or NULL */,
                                    uint8_t *coverage /* out->width * out->height bytes, or NULL */, int device, void *stream);

/* ---- multi-band blending across a camera rig: Laplacian-pyramid compose ---- */

/* FIRST leaves a step at every seam; MEAN and FEATHER trade it for a band in which the detail of two slightly misregistered
 * cameras is averaged into ghosts; gains with a realistic prior leave part of the exposure spread.  Burt and Adelson's multi-band
 * blend, as Brown and Lowe and OpenCV's MultiBandBlender use it, blends low frequencies over wide zones and high frequencies over
 * narrow ones: lrp_compose_cameras_multiband_device.  Guidance: choose num_bands so that 2^num_bands stays below the width of
 * the overlaps.  A camera's image is zero outside its coverage, as in OpenCV; nothing is filled in.
 *
 * Definition, binary32, un-fused, in the order written.  W, H, C come from `out`; B = num_bands, 0 .. 8.  The level sizes are
 * w_0 = W, w_{k+1} = (w_k + 1) >> 1, likewise h; levels 0 .. B all exist, also when a size has reached 1.
 *
 * Per pixel (level 0).  Camera i's covered_i, sx, sy and FEATHER weight w_i are exactly those of lrp_compose_cameras_device at
 * num_samples == 1.  k, the number of covering cameras, goes to `count`.  The winner is the covering camera with the largest
 * w_i: scan in ascending i, replace on w_i > best, so a tie goes to the lowest index.  `label` is the winner, or
 * LRP_MULTIBAND_NO_CAMERA when k == 0.
 *   G^i_0(x, y) is bit for bit what lrp_compose_cameras_gain_device(cams + i, 1, rotations + 9 i, gains + i, out, 1, interpolation,
 *               LRP_COMPOSE_FIRST, NULL, ...) stores for the pixel; with gains == NULL what lrp_compose_cameras_device stores.  An
 *               uncovered pixel is +0.0f.
 *   M^i_0     = (label == i) ? 1.0f : 0.0f.
 * Index rules.  Y_k(j) clamps j into 0 .. h_k - 1.  X_k(j) clamps likewise, except for an equirectangular target of a full turn
 * (the decision of the wrapping sampler, taken on out->lens), where X_k(j) is j modulo w_k, non-negative.
 * reduce (level k to k + 1, per channel and for M).  Horizontally, for x < w_{k+1}, y < h_k, with p_d = G_k(X_k(2x + d), y):
 *   h(x, y) = (((p_-2 + p_2) + 4.0f * (p_-1 + p_1)) + 6.0f * p_0) * 0.0625f
 * then the same expression vertically, on h(x, Y_k(2y + d)).
 * expand, E(T), level k + 1 to k.  In one dimension, with the neighbour indices through the index rule of level k + 1:
 *   j = 2i:      e = ((c(i - 1) + c(i + 1)) + 6.0f * c(i)) * 0.125f
 *   j = 2i + 1:  e = (c(i) + c(i + 1)) * 0.5f
 * horizontally first, which gives w_k x h_{k+1}, then vertically.
 * Laplacian and accumulation.  L^i_k = G^i_k - E(G^i_{k+1}) for k < B, L^i_B = G^i_B.  A_k,c and S_k start at +0.0f; for
 * ascending i: A_k,c = A_k,c + M^i_k * L^i_k,c (multiply, then add), S_k = S_k + M^i_k.  The product is taken as +0.0f where
 * M^i_k == 0.0f, whatever L^i_k,c is: a camera adds nothing, not even a NaN, where its weight is zero.
 * Collapse.  N_k,c = (S_k > 0.0f) ? A_k,c / S_k : +0.0f; R_B = N_B, R_k = N_k + E(R_{k+1}).  The pixel is R_0, then `post` on its
 * first min(C, 3) channels.  A pixel with label == LRP_MULTIBAND_NO_CAMERA is +0.0f in every channel, whatever post is.
 * There is no epsilon in the normalisation, so this holds exactly: with B == 0 the pixel is +0.0f + G^winner_0 — the winner's
 * one-camera render with -0.0f turned into +0.0f, whatever the other cameras hold there.  The implementation skips work only
 * where no bit changes.
 *
 * Asynchronous on `stream`; allocates nothing (the caller supplies `scratch`, DEVICE memory aligned to 256 bytes of at least
 * lrp_multiband_scratch_bytes(W, H, C, B) bytes, whose content before and after the call means nothing), does not synchronise,
 * builds no table, neither reads nor writes the geometry cache.  gains: HOST, n_in floats, or NULL.  count, label: W * H bytes
 * each, or NULL.  num_samples is 1; C is 1 .. 4; the interpolation is 0 .. 2.
 * Errors, all before a device is touched, in this order: 1. those of lrp_compose_cameras_gain_device with num_samples == 1 (no
 * mode; gains may be NULL); 2. out->channels > 4: LRP_ERR_CHANNELS; 3. num_bands outside 0 .. 8: LRP_ERR_BAD_ARG; 4. scratch
 * NULL: LRP_ERR_NULL; 5. scratch not aligned to 256 bytes, or scratch_bytes below the queried size: LRP_ERR_BAD_ARG with an
 * lrp_last_error text that states both sizes; 6. out->height above 524280 (the rows a launch grid of 8-row tiles holds):
 * LRP_ERR_BAD_DIMS.
 *
 * lrp_multiband_scratch_bytes (host only, pure): the exact size the call needs — one camera's pyramid (per level C floats per
 * texel, and above level 0 the weight plane), the accumulators A_k and S_k of every level (the collapse writes R_k over A_k), and
 * a label and a count plane, every region rounded up to 256 bytes.  Errors: bytes NULL: LRP_ERR_NULL; a size below 1:
 * LRP_ERR_BAD_DIMS; channels outside 1 .. 4: LRP_ERR_CHANNELS; num_bands outside 0 .. 8: LRP_ERR_BAD_ARG. */
#define LRP_MULTIBAND_MAX_BANDS 8
#define LRP_MULTIBAND_NO_CAMERA 255
int lrp_multiband_scratch_bytes(int width, int height, int channels, int num_bands, size_t *bytes);
int lrp_compose_cameras_multiband_device(const lrp_camera *cams, int n_in, const float *rotations /* n_in x 9, or NULL */,
                                         const float *gains /* HOST, n_in, or NULL */, const lrp_image *out, int interpolation,
                                         int num_bands, const lrp_post *post, uint8_t *count /* W * H bytes, or NULL */,
                                         uint8_t *label /* W * H bytes, or NULL */, void *scratch /* DEVICE */, size_t scratch_bytes,
                                         int device, void *stream);

/* ---- one source, several outputs, several GPUs (BASELINE configs[4]) ---------- */

/* One host source, n_out host outputs (lenses in outs[i].lens, rotations + 9 * i or none): the
 * cubemap job — six reference invocations over one 8192^2 panorama — on `n_devices` GPUs.
 * The source is uploaded ONCE, to devices[0], and copied to the other GPUs device to device
 * (hipMemcpyPeerAsync over xGMI where peer access is available, a second upload where not);
 * with n_out >= n_devices whole outputs are dealt round-robin over the GPUs (output i on
 * devices[i % n_devices]), with fewer outputs than GPUs every GPU renders band d of n_devices of
 * EVERY output (rows are independent); results are downloaded straight into outs[i].data.  No collective, no exchange of results.  The bytes are those of
 * n_out lrp_reproject calls on one GPU.  devices may name a GPU more than once. */
int lrp_reproject_multi(const lrp_image *in, lrp_image *outs, int n_out, int num_samples, int interpolation,
                        const float *rotations, const lrp_post *post, const int *devices, int n_devices);

/* ---- batches of independent images (the reference's --input-dir path) ------ */

/* A context owns a three-stage pipeline on one device — an upload stream, a
 * compute stream and a download stream, chained by events — and `n_streams`
 * image slots (device source + destination buffers, sized for the largest image
 * submitted so far).  Images are independent (src/main.cpp:540-622: one file per
 * pool thread); with n_streams >= 2 the H2D copy of image i+1, the kernel of
 * image i and the D2H copy of image i-1 run at the same time on both PCIe
 * directions (pinned host buffers make the copies asynchronous). */
typedef struct lrp_context lrp_context;

int lrp_context_create(lrp_context **ctx, int device, int n_streams);
void lrp_context_destroy(lrp_context *ctx);
/* Enqueue one image (host buffers).  Returns once the work is queued; in->data
 * must stay valid and out->data must not be read until lrp_context_wait. */
int lrp_context_submit(lrp_context *ctx, const lrp_image *in, lrp_image *out, int num_samples,
                       int interpolation, const float *rotation, const lrp_post *post);
/* Wait for everything submitted so far; returns the first error seen. */
int lrp_context_wait(lrp_context *ctx);

/* What a context does with the output pixels the source cannot see (lrp_coverage_device's mask_image / alpha_channel): applies
 * to the images submitted afterwards with lrp_context_submit and lrp_context_submit_packed.  On the image's compute stream the
 * coverage kernel follows the reprojection and its fused post_process and runs in front of the encode kernel and the download.
 * (0, -1) switches it off: the default, which leaves the pipeline as it is without this call.  An alpha_channel the image does
 * not have fails that submission with LRP_ERR_BAD_ARG. */
int lrp_context_set_outside(lrp_context *ctx, int mask_image, int alpha_channel);

/* ---- pixel formats of the file path -------------- */

/* What the reference's codecs do on the host between a file and the float buffers of the
 * hot path, done on the device so that a frame crosses PCIe in its file format (8 or 4 bytes
 * per RGBA pixel instead of 16):
 *   LRP_PIXEL_F16       interleaved IEEE binary16 — an OpenEXR HALF channel; widened exactly,
 *                       narrowed round-to-nearest-even like Imath's half
 *                       (src/image_formats.cpp:266-295, 318-333);
 *   LRP_PIXEL_U8_GAMMA  8-bit samples; decode v = pow(p / 255, 2.2) (read_png :196-198, read_jpeg
 *                       :64-66), encode uint8(255.9 * pow(clamp(v, 0, 1), 1 / 2.2)) (save_png
 *                       :155-158) — bit for bit what the host's powf gives (tables made by it).
 * Channels: the first min(src_channels, dst_channels) are converted; extra destination
 * channels are filled (decode: 0.0f; encode: `fill`, e.g. 255 for the alpha byte save_png
 * writes when the image has no fourth channel). */
typedef enum lrp_pixel_format { LRP_PIXEL_F32 = 0, LRP_PIXEL_F16 = 1, LRP_PIXEL_U8_GAMMA = 2 } lrp_pixel_format;

/* Device buffers, asynchronous on `stream`. */
int lrp_decode_pixels_device(const void *src, int src_format, int src_channels, float *dst, int dst_channels,
                             size_t n_pixels, int device, void *stream);
int lrp_encode_pixels_device(const float *src, int src_channels, void *dst, int dst_format, int dst_channels,
                             unsigned fill, size_t n_pixels, int device, void *stream);
/* The two 256-entry tables behind LRP_PIXEL_U8_GAMMA as the host's powf made them: decode[k] =
 * pow(k / 255, 2.2), threshold[k] = smallest s in [0, 1] whose code is >= k.  No device needed. */
void lrp_pixel_tables(float decode[256], float threshold[256]);

/* Page-locked host memory for the buffers handed to a context (pageable buffers work too, but
 * make every copy synchronous and half as fast).  lrp_host_free(NULL) is a no-op. */
int lrp_host_alloc(void **ptr, size_t bytes);
void lrp_host_free(void *ptr);

/* lrp_context_submit with the host buffers in a file format: in->data holds in->width x
 * in->height pixels of `in_packed_channels` samples in `in_format` (e.g. the RGBA8 libpng
 * decodes to, of which in->channels = 3 are used; or in->channels HALF samples), out->data
 * receives `out_packed_channels` samples per pixel in `out_format` (`out_fill` for channels
 * beyond out->channels).  Upload, decode kernel, reproject (+ fused post_process), encode
 * kernel, download — pipelined over the context's slots like lrp_context_submit.
 * *ticket (may be NULL) identifies the submission for lrp_context_wait_ticket, which blocks
 * until that image's output has landed while later submissions keep flowing.  A context may
 * be shared by several host threads (submissions are serialised internally). */
int lrp_context_submit_packed(lrp_context *ctx, const lrp_image *in, int in_format, int in_packed_channels,
                              lrp_image *out, int out_format, int out_packed_channels, unsigned out_fill,
                              int num_samples, int interpolation, const float *rotation, const lrp_post *post,
                              int *ticket);
int lrp_context_wait_ticket(lrp_context *ctx, int ticket);

/* ---- packed pixels: 8-bit and half images reprojected on the device by one launch -------- */

/* lrp_context_submit_packed's three kernels — decode, reproject, encode — as ONE launch on device-resident packed buffers: for a
 * caller whose frames already sit on the GPU in their real format (RGBA8 from a video decoder, binary16 from an EXR reader).
 * No float32 staging image exists: a pixel's taps are decoded as they are loaded and its value is encoded as it is stored.
 * in->data / out->data are device pointers to packed samples of any alignment, with the meaning lrp_context_submit_packed
 * gives its host pointers: in->width x in->height texels of in_packed_channels samples in in_format, out->width x out->height
 * pixels of out_packed_channels samples in out_format.  C = in->channels = out->channels (at most 8) is the channel count of
 * the float image the kernels of the chain would see.
 *
 * Definition.  The bytes written to out->data are exactly those of this chain with two float32 temporaries tmp_in, tmp_out of C
 * channels:
 *   lrp_decode_pixels_device(in->data, in_format, in_packed_channels, tmp_in, C, ...)
 *   lrp_reproject_device(tmp_in -> tmp_out, num_samples, interpolation, rotation, post)
 *   lrp_encode_pixels_device(tmp_out, C, out->data, out_format, out_packed_channels, out_fill, ...)
 * corner cases included: the channels of the source beyond in_packed_channels are +0.0f taps that go through the sampler's
 * arithmetic; packed source samples beyond C are not read; output samples beyond C are out_fill (the low 8 / 16 bits; for
 * LRP_PIXEL_F32 the fill's bit pattern); the 8-bit encode clamps with std::max(0.0f, std::min(1.0f, v)) in libstdc++'s
 * comparison direction — NaN becomes 255, -0 becomes 0 —; num_samples <= 0 leaves out->data untouched.  Nothing new is
 * defined about arithmetic: the 8-bit decode is the 256-entry table and the encode the search of the 255 thresholds of
 * lrp_pixel_tables, the half conversions are include/lrp_half.h.  One thing the chain leaves open is settled here: where a
 * sample of the chain is a NaN (a NaN or an infinity among the taps), its sign and payload are those of the chain whose
 * lrp_reproject_device renders with the one-pixel-per-lane kernels (lrp_debug_kernel(0)) — the samplers this call runs.
 * The kernel families of lrp_reproject_device agree among themselves on every bit but these (their blends associate
 * differently and a NaN keeps the sign of the operand it came from); an 8-bit output has no NaN (it is 255).
 *
 * in_format is LRP_PIXEL_F16 or LRP_PIXEL_U8_GAMMA (a float32 source needs no decode: lrp_reproject_device +
 * lrp_encode_pixels_device); out_format is any of the three.
 *
 * Asynchronous on `stream`.  The first call on a device uploads the two 8-bit tables (2 KiB, one synchronisation, like the
 * conversion kernels).  A num_samples == 1 call goes through the geometry cache under the key of lrp_reproject_device for the
 * same geometry: the first launch writes the coordinate map as a side output, later ones — of either entry point — load it
 * (lrp_geometry_cache_stats: fills / hits); a capturing stream, a switched-off cache or lrp_debug_set("geo_cache", 0) compute.
 * Errors, all before a device is touched, in this order: in or out NULL: LRP_ERR_NULL; the checks of lrp_reproject_device in
 * its order and with its statuses (lens and extension bits, interpolation, channels, sizes, data pointers); LRP_ERR_BAD_ARG
 * for in_format == LRP_PIXEL_F32, an unknown format or a packed channel count < 1; LRP_ERR_CHANNELS for C > 8;
 * LRP_ERR_BAD_DIMS for a packed image — width x height x packed channels x bytes per sample — of more than 2^31 bytes (the
 * kernel forms 32-bit byte offsets). */
int lrp_reproject_packed_device(const lrp_image *in, int in_format, int in_packed_channels, lrp_image *out, int out_format,
                                int out_packed_channels, unsigned out_fill, int num_samples, int interpolation,
                                const float *rotation, const lrp_post *post, int device, void *stream);

/* ---- compose, packed pixels: 8-bit and half sources composed into a packed output by one launch -------- */

/* lrp_compose_device on sources and an output in their real formats: the frames of a camera rig — RGBA8 from a video decoder,
 * binary16 from an EXR reader —, several of them, stitched into one 8-bit, binary16 or float output by ONE launch.  No float32
 * staging image exists: a source's taps are decoded as they are loaded and the composed value is encoded as it is stored.
 * ins[i].data / out->data are device pointers to packed samples of any alignment (each source's own), with the meaning
 * lrp_reproject_packed_device gives them: ins[i].width x ins[i].height texels of in_packed_channels samples in in_format — one
 * format and one packed channel count for all sources —, out->width x out->height pixels of out_packed_channels samples in
 * out_format.  C = ins[i].channels = out->channels (at most 8) is the channel count of the float images the kernels of the
 * chain would see.  Sizes, lens parameters and rotations differ per source, as in lrp_compose_device.
 *
 * Definition.  The bytes written to out->data and to count are exactly those of this chain with float32 temporaries tmp_i (one
 * per source) and tmp_out, each of C channels:
 *   for each i:  lrp_decode_pixels_device(ins[i].data, in_format, in_packed_channels, tmp_i, C, ...)
 *   lrp_compose_device(tmp_0 .. tmp_{n_in - 1} -> tmp_out, rotations, interpolation, mode, post, count)
 *   lrp_encode_pixels_device(tmp_out, C, out->data, out_format, out_packed_channels, out_fill, ...)
 * the corner cases of both parents included: the channels of a source beyond in_packed_channels are +0.0f taps that go through
 * the sampler's arithmetic; packed source samples beyond C are not read; output samples beyond C are out_fill (the low 8 / 16
 * bits; for LRP_PIXEL_F32 the fill's bit pattern), also for a pixel no source covers; such a k == 0 pixel is +0.0f in the first
 * C channels before the encode, whatever post is (code 0 for 8-bit); the 8-bit encode clamps as lrp_encode_pixels_device does —
 * NaN becomes 255, -0 becomes 0.  Nothing new is defined about arithmetic.  Where a sample of the chain is a NaN (a NaN or an
 * infinity among the taps of a half source, or inf - inf in a blend), its sign and payload are the chain's; an 8-bit source
 * cannot produce a NaN, an 8-bit output has none.
 *
 * in_format is LRP_PIXEL_F16 or LRP_PIXEL_U8_GAMMA (float32 sources need no decode: lrp_compose_device +
 * lrp_encode_pixels_device); out_format is any of the three.
 *
 * Asynchronous on `stream`; allocates nothing, builds no lens table, neither reads nor writes the geometry cache (the
 * lrp_geometry_cache_stats counters do not move).  The first call on a device uploads the two 8-bit tables (2 KiB, one
 * synchronisation, like the conversion kernels and lrp_reproject_packed_device, whose copy it shares).
 * Errors, all before a device is touched, in this order: the errors of lrp_compose_device in its order and with its statuses
 * and texts (n_in / mode; NULL; per source the checks of lrp_reproject_device(ins + i, out) with interpolation 0 .. 2 only; the
 * mix of source modes); LRP_ERR_BAD_ARG for in_format == LRP_PIXEL_F32, an unknown format or a packed channel count < 1;
 * LRP_ERR_CHANNELS for C > 8; LRP_ERR_BAD_DIMS for a packed image — a source or the output: width x height x packed channels x
 * bytes per sample — of more than 2^31 bytes (the kernel forms 32-bit byte offsets). */
int lrp_compose_packed_device(const lrp_image *ins, int n_in, int in_format, int in_packed_channels,
                              const float *rotations /* n_in x 9, or NULL */, const lrp_image *out, int out_format,
                              int out_packed_channels, unsigned out_fill, int interpolation, int mode, const lrp_post *post,
                              uint8_t *count /* out->width * out->height bytes, or NULL */, int device, void *stream);

/* ---- calibrated cameras, packed pixels: a rig's 8-bit and half frames measured and stitched with no float32 image -------- */

/* lrp_compose_cameras_gain_device and lrp_camera_overlap_device on frames in their real formats.  cams[i].data carries a device
 * pointer to packed samples of any alignment (each camera's own), cast to the field's type: cams[i].width x cams[i].height
 * texels of in_packed_channels samples in in_format — one format and one packed channel count for all cameras.  out->data
 * likewise: out->width x out->height pixels of out_packed_channels samples in out_format.  C = out->channels (at most 8) is the
 * channel count of the float images the kernels of the chain would see.
 *
 * lrp_compose_cameras_packed_device.  The bytes written to out->data, count and coverage are exactly those of this chain with
 * float32 temporaries tmp_i (one per camera) and tmp_out, each of C channels:
 *   for each i:  lrp_decode_pixels_device(cams[i].data, in_format, in_packed_channels, tmp_i, C, ...)
 *   lrp_compose_cameras_gain_device(tmp_0 .. -> tmp_out, rotations, gains, num_samples, interpolation, mode, post, count,
 *                                   coverage) — lrp_compose_cameras_device where gains is NULL
 *   lrp_encode_pixels_device(tmp_out, C, out->data, out_format, out_packed_channels, out_fill, ...)
 * with the corner cases of lrp_compose_packed_device word for word: +0.0f taps behind in_packed_channels; out_fill behind C,
 * also on a pixel no sub-sample of which is covered; such an m == 0 pixel is +0.0f (code 0) whatever post is; the 8-bit clamp
 * maps NaN to 255 and -0 to 0; a NaN's sign and payload are the chain's, except that a call without gains multiplies by 1.0f,
 * which leaves every value but a signalling NaN's quiet bit as it is (an 8-bit source cannot produce a NaN).
 * gains is a HOST array of n_in floats, read before the call returns, or NULL.  in_format is LRP_PIXEL_F16 or
 * LRP_PIXEL_U8_GAMMA; out_format is any of the three.  One launch.  Asynchronous on `stream`; allocates nothing, builds no
 * table, neither reads nor writes the geometry cache; shares the device copy of the two 8-bit tables with the other packed calls
 * (the first call on a device uploads it).
 * Errors, all before a device is touched, in this order: items 1 to 5 of lrp_compose_cameras_device with their statuses and
 * texts; LRP_ERR_BAD_ARG, naming the camera, for a gain that is not finite or is negative; item 6 (num_samples);
 * LRP_ERR_BAD_ARG for in_format == LRP_PIXEL_F32 (float32 frames: lrp_compose_cameras_device or
 * lrp_compose_cameras_gain_device, then lrp_encode_pixels_device), an unknown format or a packed channel count < 1;
 * LRP_ERR_CHANNELS for C > 8; LRP_ERR_BAD_DIMS for a packed frame or output of more than 2^31 bytes.
 *
 * lrp_camera_overlap_packed_device.  The LRP_OVERLAP_WORDS words written to stats (DEVICE) are, as integers, those of
 * lrp_decode_pixels_device per camera -> lrp_camera_overlap_device(.., out, lo, hi, stats); of `out` the lens, the size and
 * channels (C) are read.  The table feeds lrp_camera_gains unchanged.  Errors: those of lrp_camera_overlap_device in its order,
 * then the packed errors above (format, packed channel count, C > 8, frame size). */
int lrp_compose_cameras_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels,
                                      const float *rotations /* n_in x 9, or NULL */, const float *gains /* HOST, n_in, or NULL */,
                                      const lrp_image *out, int out_format, int out_packed_channels, unsigned out_fill,
                                      int num_samples, int interpolation, int mode, const lrp_post *post,
                                      uint8_t *count, uint8_t *coverage, int device, void *stream);
int lrp_camera_overlap_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels,
                                     const float *rotations /* n_in x 9, or NULL */, const lrp_image *out /* lens, size, channels */,
                                     float lo, float hi, uint64_t *stats /* DEVICE, LRP_OVERLAP_WORDS */, int device, void *stream);

/* ---- multi-band blending, packed pixels: the blend of a rig's 8-bit and half frames with no float32 frame or panorama ------ */

/* lrp_compose_cameras_multiband_device on frames and an output in their real formats; with lrp_camera_overlap_packed_device and
 * lrp_camera_gains the chain overlap -> gains -> blend runs without a float32 copy of any frame.  cams[i].data and out->data carry
 * packed device pointers of any alignment, as in lrp_compose_cameras_packed_device: cams[i].width x cams[i].height texels of
 * in_packed_channels samples in in_format, out->width x out->height pixels of out_packed_channels samples in out_format.
 * C = out->channels, 1 .. 4; num_samples is 1.
 *
 * Definition.  The bytes written to out->data, count and label are exactly those of this chain with float32 temporaries tmp_i
 * (one per camera) and tmp_out, each of C channels:
 *   for each i:  lrp_decode_pixels_device(cams[i].data, in_format, in_packed_channels, tmp_i, C, ...)
 *   lrp_compose_cameras_multiband_device(tmp_0 .. -> tmp_out, rotations, gains, interpolation, num_bands, post, count, label,
 *                                        scratch, ...)
 *   lrp_encode_pixels_device(tmp_out, C, out->data, out_format, out_packed_channels, out_fill, ...)
 * with the corner cases of lrp_compose_cameras_packed_device word for word: +0.0f taps behind in_packed_channels; out_fill behind
 * C, also on a pixel with label == LRP_MULTIBAND_NO_CAMERA; such a pixel is +0.0f (code 0) in its first C channels whatever post
 * is; the 8-bit clamp maps NaN to 255 and -0 to 0.  A NaN's sign and payload are the chain's: a camera's level-0 layer is
 * lrp_compose_cameras_packed_device's with one camera, which multiplies by 1.0f where gains is NULL, but every G_0 value that
 * reaches the output has passed M * L and an addition on both routes, which quiet a signalling NaN alike.
 * in_format is LRP_PIXEL_F16 or LRP_PIXEL_U8_GAMMA; out_format is any of the three.
 *
 * scratch: what the float call needs — DEVICE memory aligned to 256 bytes of at least lrp_multiband_scratch_bytes(W, H, C, B)
 * bytes; the pyramid stays float32.  The launches are the float call's, except that a camera's level-0 layer comes from the
 * one-camera packed compose kernel and the last launch, the level-0 collapse, encodes.  Asynchronous on `stream`; allocates
 * nothing, neither reads nor writes the geometry cache; shares the device copy of the two 8-bit tables with the other packed
 * calls (the first packed call on a device uploads it: the one synchronisation).  gains: HOST, n_in floats, or NULL.
 * Errors, all before a device is touched, in this order: items 1 to 6 of lrp_compose_cameras_multiband_device with their
 * statuses and texts; then the packed items of lrp_compose_cameras_packed_device in its order: LRP_ERR_BAD_ARG for
 * in_format == LRP_PIXEL_F32 (float32 frames: lrp_compose_cameras_multiband_device, then lrp_encode_pixels_device), an unknown
 * format or a packed channel count < 1; LRP_ERR_BAD_DIMS for a packed frame or output of more than 2^31 bytes; then, this
 * call's own, LRP_ERR_BAD_DIMS where W * H * C * 4 exceeds 2^31 bytes: a camera's level-0 layer is a float32 image of C samples
 * per pixel in the scratch, up to four times the size of the packed output, and the packed camera kernel that writes it forms
 * 32-bit byte offsets (C == 4: at most 2^27 pixels, e.g. 16384 x 8192). */
int lrp_compose_cameras_multiband_packed_device(const lrp_camera *cams, int n_in, int in_format, int in_packed_channels,
                                                const float *rotations /* n_in x 9, or NULL */,
                                                const float *gains /* HOST, n_in, or NULL */, const lrp_image *out, int out_format,
                                                int out_packed_channels, unsigned out_fill, int interpolation, int num_bands,
                                                const lrp_post *post, uint8_t *count /* W * H bytes, or NULL */,
                                                uint8_t *label /* W * H bytes, or NULL */, void *scratch /* DEVICE */,
                                                size_t scratch_bytes, int device, void *stream);

/* ---- Lanczos-3---------------------------------------------------------------------------- */

/* LRP_LANCZOS3 (interpolation 3, with LRP_SAMPLER_EXT_LANCZOS3 on): a fourth sampler with a 6 x 6 footprint, the filter that
 * ffmpeg v360, Hugin, OpenCV and Pillow offer under this name.  The reference has none, so this text is the definition.
 *
 * Accepted by every entry point that renders through lrp_reproject_device's launcher: lrp_reproject, lrp_reproject_device,
 * lrp_reproject_rows_device, lrp_reproject_batch_device, lrp_reproject_multi_device, lrp_reproject_multi,
 * lrp_context_submit, lrp_context_submit_packed.  With the bit off they return LRP_ERR_INTERPOLATION where the reference's
 * interpolation check stands in the validation order.  lrp_compose_device, lrp_compose_packed_device and
 * lrp_reproject_packed_device reject interpolation 3 at that position whether the bit is on or off.
 *
 * All arithmetic is binary32, un-fused, in the order written.  sinf_ and cosf_ are the glibc clones of lrp_math.h (the same
 * bits on host and device).  trunc_x86 (int(float) as cvttss2si: NaN, infinities and out-of-range give INT_MIN),
 * column<Loop> (wrapping sources wrap, others clamp), clamp_index and unit_clamp (std::max(0.0f, std::min(1.0f, v)) in
 * libstdc++'s comparison direction: NaN -> 1) are those of the bicubic sampler.  kPi = 0x1.921fb6p+1f,
 * kSin60 = 0x1.bb67aep-1f.  (sx, sy) are the top-left-origin source coordinates every sampler receives.
 *
 * Taps, k = -2 .. 3:   ix_k = column<Loop>(trunc_x86(sx + (float)k), in_w)   (k = 0: trunc_x86(sx))
 *                      iy_k = clamp_index(trunc_x86(sy + (float)k), in_h - 1)
 *                      fx = unit_clamp(sx - (float)ix_0),  fy = unit_clamp(sy - (float)iy_0)
 * — the fractions come from the clamped index, as in the reference's bicubic.
 *
 * Half weights  half(t) -> h0, h1, h2  for the distances t, t + 1, t + 2:
 *   p = kPi * t;  s = sinf_(p);  q = p / 3.0f;  s3 = sinf_(q);  c3 = cosf_(q)
 *   h0 = (p == 0.0f) ? 1.0f : (3.0f * (s / p)) * (s3 / p)
 *   p1 = kPi * (t + 1.0f);  a1 = (0.5f * s3) + (kSin60 * c3);  h1 = (3.0f * ((-s) * a1)) / (p1 * p1)
 *   p2 = kPi * (t + 2.0f);  a2 = (kSin60 * c3) - (0.5f * s3);  h2 = (3.0f * (s * a2)) / (p2 * p2)
 * i.e. sinc(d) sinc(d / 3) with sin(pi (t + j)) = +-sin(pi t) and sin(pi (t + j) / 3) from the angle sum: two
 * trigonometric calls per half instead of six.
 *
 * Axis weights from f:  f == 0.0f: {0, 0, 1, 0, 0, 0};  f == 1.0f: {0, 0, 0, 1, 0, 0}  (+0.0f and 1.0f);  otherwise
 *   L = half(f), R = half(1.0f - f);  r = {L2, L1, L0, R0, R1, R2}  (tap order k = -2 .. 3)
 *   W = ((((r0 + r1) + r2) + r3) + r4) + r5;  w_k = r_k / W
 * The right-hand taps use 1 - f, so the weight next to the nearest tap stays accurate on both sides.
 *
 * Blend, vertical per tap column and then horizontal, like bicubicInterpolate; p(i, j) is the texel at (ix_i, iy_j):
 *   per tap column i and channel:  col_i = wy_0 * p(i, 0);  col_i = col_i + wy_j * p(i, j)  for j = 1 .. 5
 *   out = wx_0 * col_0;  out = out + wx_i * col_i  for i = 1 .. 5          (each step a multiply, then an add)
 * Sub-samples (acc = 0; acc += out, ssx outer, ssy inner), normalize, the fused post and the channel rules are those of
 * every other sampler.
 *
 * A num_samples == 1 call of a whole image goes through the geometry cache under the key of the other samplers: entries are
 * shared with them in both directions. */

/* ---- synthetic frames (bench / tests) -------------------------------------- */

/* Fill a device buffer with the counter-based synthetic frame of SURVEY.md §8d
 * (identical bits to oracle lrpo_synth_fill on the host).  depth_channel = -1
 * for colour-only frames. */
int lrp_synth_fill_device(float *data, int width, int height, int channels, uint32_t seed,
                          int depth_channel, int device, void *stream);

/* Order-independent 64-bit checksum of the bit patterns of n floats on the device, written to
 * the device word *out (asynchronous on `stream`): sum mod 2^64 of h(bits[i], i) with
 * h = mix32(bits ^ 0xA5A5A5A5, 2 i + 0x7F4A7C15) << 32 | mix32(bits, i), mix32 as in the
 * synthetic generator.  bench.py and the multi-GPU tests compare per-image values between
 * 1-rank and N-rank runs without moving the images. */
int lrp_checksum_device(const float *data, size_t n, uint64_t *out, int device, void *stream);

/* Evaluate the device math routines on device arrays (lets tests prove the
 * device build of the math matches the host libm): func 0 sinf, 1 cosf,
 * 2 sincosf.sin, 3 sincosf.cos, 4 atanf, 5 asinf, 6 atan2f(a, b), 7 a / b,
 * 8 sqrtf(a), 9 (float)int(a) with the x86 cvttss2si convention.
 * `b` may be NULL for unary functions. */
int lrp_math_eval_device(int func, const float *a, const float *b, float *out, size_t n, int device,
                         void *stream);

/* ---- caller-side producers of hot-path inputs (host, no device needed) ------ */

/* computeRotationMatrix (reference src/main.cpp:98-142): R = R_y(pan) * R_x(pitch)
 * * R_z(roll), row-major, angles in radians, float sin/cos. */
void lrp_rotation_matrix(float pan, float pitch, float roll, float *out9);

/* Lens constructors with the reference CLI's conventions (src/main.cpp:15-95):
 * rectilinear: sensor_height = res_y / res_x * sensor_width (:27);
 * equidistant: sensor 36 x 36 mm (:53-54);
 * equirectangular: sensor 0 (:93); lrp_lens_equirectangular_full = "full"
 * (-pi..pi, -pi/2..pi/2 narrowed to float, :62-66). */
void lrp_lens_rectilinear(lrp_lens *lens, float focal_length, float sensor_width, float res_x, float res_y);
void lrp_lens_equidistant(lrp_lens *lens, float fov);
void lrp_lens_equirectangular(lrp_lens *lens, float longitude_min, float longitude_max, float latitude_min,
                              float latitude_max);
void lrp_lens_equirectangular_full(lrp_lens *lens);
/* equisolid (the LRP_LENS_EXT_EQUISOLID extension): sensor_height = res_y / res_x * sensor_width, as the CLI's --equisolid
 * (src/main.cpp:45); fov is carried, not used by the mapping. */
void lrp_lens_equisolid(lrp_lens *lens, float focal_length, float sensor_width, float fov, float res_x, float res_y);
/* stereographic (the LRP_LENS_EXT_STEREOGRAPHIC extension): sensor_height = res_y / res_x * sensor_width, like the equisolid lens. */
void lrp_lens_stereographic(lrp_lens *lens, float focal_length, float sensor_width, float res_x, float res_y);

#ifdef __cplusplus
}
#endif
#endif /* LRP_H */
