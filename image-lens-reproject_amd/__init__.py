"""image-lens-reproject_amd — MI355X-native lens reprojection (hot path only).

Python mirror of the reference operator interface (reference src/reproject.hpp:7-27,
src/config.hpp:7-37): same names and argument meaning —

    reproject(in_image, out_image, num_samples, interpolation, rotation_matrix)
    post_process(image, exposure, reinhard)
    test_conversion_math()

over the C ABI of include/lrp.h (liblrp_hip.so, hand-written HIP for gfx950).
Image data may be a C-contiguous float32 numpy array (host path: upload, kernel,
download) or a float32 torch CUDA tensor (device-resident path, asynchronous on
the given / current torch stream).  There is no CPU implementation here: without
the HIP library and a GPU every compute call raises.  Beyond the reference:
coverage(in_image, out_image, num_samples, rotation_matrix) tells which output
pixels the source image can see (device tensors), and
compose(in_images, out_image, interpolation, rotation_matrices, mode) renders
several source images into one output (device tensors), and
compose_ss(in_images, out_image, num_samples, interpolation, ...) does so with
num_samples^2 sub-samples per pixel (anti-aliased stitching), and
compose_cameras(cameras, out_image, num_samples, interpolation, ...) takes the
frames of calibrated cameras (Camera: fx, fy, cx, cy and Brown-Conrady or
Kannala-Brandt distortion coefficients) instead of ideal lenses, and
camera_view(cameras, target, out, num_samples, interpolation, ...) renders them
into the frame of another calibrated camera (camera_unproject(camera, uv) is
the pixel-to-ray inverse it uses, on the host), and
camera_overlap(cameras, out_image, ...) -> camera_gains(stats, n) ->
compose_cameras(..., gains=g) match the cameras' exposures: the statistic of the
pairwise overlaps by one launch, gain compensation on the host, and compose with
one gain per camera; camera_overlap_packed(...) and compose_cameras_packed(...)
do the same on 8-bit and half frames, with no float32 image in between.
compose_cameras_multiband(cameras, out_image, interpolation, ...) blends the
cameras over a Laplacian pyramid (multi-band blending) instead of per pixel.
compose_cameras_multiband_packed(...) does that on 8-bit and half frames into a
packed output, again with no float32 frame or panorama.

The directory name contains a hyphen (it is the name the build contract fixes);
import it with importlib.import_module("image-lens-reproject_amd").
"""
import ctypes
import enum

import numpy as np

from . import _native
from ._native import LrpImage, LrpLens, LrpPost


class LensType(enum.IntEnum):  # reference src/config.hpp:7-13
    RECTILINEAR = 0
    FISHEYE_EQUIDISTANT = 1
    FISHEYE_EQUISOLID = 2
    FISHEYE_STEREOGRAPHIC = 3
    EQUIRECTANGULAR = 4


class Interpolation(enum.IntEnum):  # reference src/reproject.hpp:16-20
    NEAREST = 0
    BILINEAR = 1
    BICUBIC = 2


class DataLayout(enum.IntEnum):  # reference src/reproject.hpp:7
    RGB = 0
    RGBA = 1
    RGBZ = 2
    RGBAZ = 3


class Status(enum.IntEnum):
    OK = 0
    OUTPUT_LENS = 1
    INPUT_LENS = 2
    INTERPOLATION = 3
    CHANNELS = 4
    BAD_DIMS = 5
    NULL = 6
    NO_DEVICE = 7
    HIP = 8
    OOM = 9
    BAD_ARG = 10


class ComposeMode(enum.IntEnum):  # include/lrp.h lrp_compose_mode
    FIRST = 0
    MEAN = 1
    FEATHER = 2


COMPOSE_MAX_SOURCES = 8  # include/lrp.h LRP_COMPOSE_MAX_SOURCES


class LrpError(RuntimeError):
    """A non-zero lrp_status.  For the three dispatch failures the message is the
    exact line the reference prints before exit(1) (src/reproject.cpp:365,396,416)."""

    def __init__(self, status, detail=""):
        self.status = Status(status) if status in Status._value2member_map_ else status
        lib = _native.load()
        base = lib.lrp_strerror(int(status)).decode()
        super().__init__(f"{base} [{detail}]" if detail and detail != base else base)


def _check(status):
    if status != 0:
        raise LrpError(status, _native.load().lrp_last_error().decode())


class LensInfo:
    """reference struct LensInfo (src/config.hpp:15-37).  Units: mm, radians."""

    def __init__(self, type, params=(0.0, 0.0, 0.0, 0.0), sensor_width=0.0, sensor_height=0.0):
        self.type = int(type)
        p = list(params) + [0.0] * (4 - len(params))
        self.params = [float(np.float32(v)) for v in p]
        self.sensor_width = float(np.float32(sensor_width))
        self.sensor_height = float(np.float32(sensor_height))

    @classmethod
    def _from_c(cls, c):
        return cls(c.type, list(c.raw), c.sensor_width, c.sensor_height)

    @classmethod
    def rectilinear(cls, focal_length, sensor_width, res_x, res_y):
        """--rectilinear focal_len,sensor_width (src/main.cpp:15-29)."""
        c = LrpLens()
        _native.load().lrp_lens_rectilinear(ctypes.byref(c), focal_length, sensor_width, res_x, res_y)
        return cls._from_c(c)

    @classmethod
    def equidistant(cls, fov):
        """--equidistant fov (src/main.cpp:49-56)."""
        c = LrpLens()
        _native.load().lrp_lens_equidistant(ctypes.byref(c), fov)
        return cls._from_c(c)

    @classmethod
    def equisolid(cls, focal_length, sensor_width, fov, res_x, res_y):
        """--equisolid focal_len,sensor_width,fov (src/main.cpp:31-46): sensor_height = res_y / res_x * sensor_width.
        Renders only while the LENS_EXT_EQUISOLID extension is on (lens_extensions)."""
        c = LrpLens()
        _native.load().lrp_lens_equisolid(ctypes.byref(c), focal_length, sensor_width, fov, res_x, res_y)
        return cls._from_c(c)

    @classmethod
    def stereographic(cls, focal_length, sensor_width, res_x, res_y):
        """--stereographic focal_len,sensor_width: r = 2 f tan(theta / 2) (include/lrp.h); sensor_height = res_y / res_x *
        sensor_width.  Renders only while the LENS_EXT_STEREOGRAPHIC extension is on (lens_extensions)."""
        c = LrpLens()
        _native.load().lrp_lens_stereographic(ctypes.byref(c), focal_length, sensor_width, res_x, res_y)
        return cls._from_c(c)

    @classmethod
    def equirectangular(cls, longitude_min=None, longitude_max=None, latitude_min=None, latitude_max=None):
        """--equirectangular full | lon_min,lon_max,lat_min,lat_max (src/main.cpp:58-95)."""
        c = LrpLens()
        lib = _native.load()
        if longitude_min is None:
            lib.lrp_lens_equirectangular_full(ctypes.byref(c))
        else:
            lib.lrp_lens_equirectangular(ctypes.byref(c), longitude_min, longitude_max, latitude_min, latitude_max)
        return cls._from_c(c)

    def to_c(self):
        c = LrpLens()
        c.type = self.type
        for i in range(4):
            c.raw[i] = self.params[i]
        c.sensor_width = self.sensor_width
        c.sensor_height = self.sensor_height
        return c


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class Image:
    """reference struct Image (src/reproject.hpp:9-14): lens + width/height/channels +
    interleaved float32 data[(y*W + x)*C + c]."""

    def __init__(self, lens, width, height, channels, data=None, data_layout=DataLayout.RGBA):
        self.lens = lens
        self.width = int(width)
        self.height = int(height)
        self.channels = int(channels)
        self.data = data
        self.data_layout = int(data_layout)

    def _ptr(self):
        d = self.data
        if d is None:
            return None
        n = self.width * self.height * self.channels
        if _is_torch(d):
            import torch

            if d.dtype != torch.float32 or not d.is_contiguous() or d.numel() != n:
                raise ValueError("image tensor must be contiguous float32 with width*height*channels elements")
            return d.data_ptr()
        if not isinstance(d, np.ndarray) or d.dtype != np.float32 or not d.flags["C_CONTIGUOUS"] or d.size != n:
            raise ValueError("image array must be C-contiguous float32 with width*height*channels elements")
        return d.ctypes.data

    def on_device(self):
        return _is_torch(self.data) and self.data.is_cuda

    def to_c(self):
        c = LrpImage()
        c.lens = self.lens.to_c()
        c.width, c.height, c.channels = self.width, self.height, self.channels
        c.data = self._ptr()
        c.data_layout = self.data_layout
        return c


def _rotation_arg(rotation_matrix):
    if rotation_matrix is None:
        return None, None
    r = np.ascontiguousarray(np.asarray(rotation_matrix, dtype=np.float32).reshape(9))
    return r, r.ctypes.data


def _rotations_arg(rotation_matrices, n):
    """_rotation_arg for n matrices, one per source or output: (the array to keep alive across the call, its address)."""
    if rotation_matrices is None:
        return None, None
    r = np.ascontiguousarray(np.asarray(rotation_matrices, dtype=np.float32).reshape(n, 9))
    return r, r.ctypes.data


def _post_arg(post):
    """post=(exposure, reinhard) or None: (the LrpPost to keep alive across the call, its reference or None)."""
    if post is None:
        return None, None
    cpost = LrpPost(float(post[0]), float(post[1]))
    return cpost, ctypes.byref(cpost)


def _gains_arg(gains, n):
    """One gain per camera, a tensor or anything numpy takes, or None: (the float32 array to keep alive across the call, its
    address)."""
    if gains is None:
        return None, None
    g = np.ascontiguousarray(np.asarray(gains.cpu() if _is_torch(gains) else gains, dtype=np.float32).reshape(-1))
    if g.size != n:
        raise ValueError("gains must hold one value per camera")
    return g, g.ctypes.data


def _plane_error(name):
    return ValueError(f"{name} must be a contiguous uint8 CUDA tensor with height*width elements")


def _check_planes(height, width, **planes):
    """The plane arguments of a compose call (count / coverage / label), each None or False (not wanted), True (allocate one) or
    a tensor to fill, which is checked here — before the call looks at its images; _alloc_planes, once the device is known,
    makes the planes."""
    for name, arg in planes.items():
        if arg is None or arg is False or arg is True:
            continue
        import torch

        if not _is_torch(arg) or arg.dtype != torch.uint8 or not arg.is_cuda or not arg.is_contiguous() or arg.numel() != height * width:
            raise _plane_error(name)


def _alloc_planes(height, width, device, *planes):
    """Per plane argument (after _check_planes): None, the caller's tensor, or a new (height, width) uint8 tensor on `device`."""
    out = []
    for arg in planes:
        if arg is True:
            import torch

            arg = torch.empty((height, width), dtype=torch.uint8, device=f"cuda:{device}")
        out.append(None if arg is None or arg is False else arg)
    return out


def _data_ptr(tensor):
    return tensor.data_ptr() if tensor is not None else None


def _check_stats(stats):
    """The overlap table of a camera_overlap call, where the caller passes one."""
    if stats is None:
        return
    import torch

    if not _is_torch(stats) or stats.dtype != torch.int64 or not stats.is_cuda or not stats.is_contiguous() or stats.numel() != 128:
        raise ValueError("stats must be a contiguous int64 CUDA tensor with 8*8*2 elements")


def _stats_arg(stats, device):
    """The caller's table (after _check_stats), or a new one on `device`."""
    if stats is not None:
        return stats
    import torch

    return torch.empty((8, 8, 2), dtype=torch.int64, device=f"cuda:{device}")


def _scratch_arg(scratch, out_image, num_bands, device):
    """The scratch of a multi-band call: the caller's tensor, checked (its size and alignment are the library's to check), or a
    new one of multiband_scratch_bytes(...) bytes on `device`."""
    import torch

    if scratch is None:
        return torch.empty(multiband_scratch_bytes(out_image.width, out_image.height, out_image.channels, num_bands), dtype=torch.uint8,
                           device=f"cuda:{device}")
    if not _is_torch(scratch) or scratch.dtype != torch.uint8 or not scratch.is_cuda or not scratch.is_contiguous():
        raise ValueError("scratch must be a contiguous uint8 CUDA tensor")
    return scratch


def _stream_handle(stream):
    if stream is None:
        import torch

        return torch.cuda.current_stream().cuda_stream
    if hasattr(stream, "cuda_stream"):
        return stream.cuda_stream
    return int(stream)


def rotation_matrix(pan, pitch, roll):
    """computeRotationMatrix (src/main.cpp:110-142); radians; row-major 9 floats."""
    out = (ctypes.c_float * 9)()
    _native.load().lrp_rotation_matrix(pan, pitch, roll, out)
    return np.array(out, dtype=np.float32)


def device_count():
    return _native.load().lrp_device_count()


PIXEL_KERNEL, TILE_KERNEL, WINDOW_KERNEL = 0, 1, 2


def debug_kernel(choice=-1):
    """lrp_debug_kernel: select the HIP kernel family (0 pixel, 1 tile, 2 tile + LDS-window
    bicubic, 3 the same without shared tap coefficients; all produce the same bits);
    returns the previous choice.  -1 only queries."""
    return _native.load().lrp_debug_kernel(int(choice))


LENS_EXT_EQUISOLID = 1  # include/lrp.h LRP_LENS_EXT_EQUISOLID
LENS_EXT_STEREOGRAPHIC = 0x100  # include/lrp.h LRP_LENS_EXT_STEREOGRAPHIC


def lens_extensions(mask=None):
    """lrp_lens_extensions: the process-wide mask of opt-in lens extensions (0 by default: the reference's lenses only).
    Sets it and returns the previous mask; None only queries."""
    return _native.load().lrp_lens_extensions(-1 if mask is None else int(mask))


LANCZOS3 = 3  # include/lrp.h LRP_LANCZOS3: an interpolation value outside Interpolation (the reference's enum keeps its three members)
SAMPLER_EXT_LANCZOS3 = 1  # include/lrp.h LRP_SAMPLER_EXT_LANCZOS3


def sampler_extensions(mask=None):
    """lrp_sampler_extensions: the process-wide mask of opt-in sampler extensions (0 by default: interpolation LANCZOS3 is
    rejected like any unknown value).  Sets the mask and returns the previous one; None only queries."""
    return _native.load().lrp_sampler_extensions(-1 if mask is None else int(mask))


def debug_set(name, value=-1):
    """lrp_debug_set: the named A/B switch ("xsep", "quad", "mirror_modes", "win_edge", "win_split", "geo_cache",
    "batch_frames", "multi_fork", "geo_strip", "geo_big", "geo_lists", "geo_fill_stream", "geo_fill_fused", "kernel"; "listed_launches" is a
    counter); returns the previous value, -1 only queries."""
    prev = _native.load().lrp_debug_set(str(name).encode(), int(value))
    if prev < 0:
        raise ValueError(f"unknown debug switch {name!r}")
    return prev


def geometry_cache_configure(max_bytes=-1, min_sightings=-1):
    """lrp_geometry_cache_configure: bytes per device (0 switches the cache off and frees it), launches of a geometry
    before it is cached; negative values keep the current setting."""
    _check(_native.load().lrp_geometry_cache_configure(int(max_bytes), int(min_sightings)))


def geometry_cache_stats():
    """lrp_geometry_cache_stats as a dict: bytes, max_bytes, entries, fills, hits, bypasses, evictions."""
    info = _native.LrpGeometryCacheInfo()
    _native.load().lrp_geometry_cache_stats(ctypes.byref(info))
    return {n: int(getattr(info, n)) for n, _ in info._fields_}


def release_cached_tables():
    """lrp_release_cached_tables: frees the lens tables and the geometry cache of every device."""
    _native.load().lrp_release_cached_tables()


def reproject(in_image, out_image, num_samples, interpolation, rotation_matrix=None, post=None, device=None,
              stream=None):
    """reproject::reproject (src/reproject.cpp:405-419).  `post=(exposure, reinhard)`
    fuses post_process into the store.  Device tensors: asynchronous on `stream`
    (default: torch's current stream); numpy arrays: synchronous."""
    lib = _native.load()
    cin, cout = in_image.to_c(), out_image.to_c()
    keep, rot = _rotation_arg(rotation_matrix)
    cpost, ppost = _post_arg(post)
    if in_image.on_device() != out_image.on_device():
        raise ValueError("input and output image data must both be on the host or both on the device")
    if in_image.on_device():
        dev = in_image.data.device.index if device is None else device
        st = lib.lrp_reproject_device(ctypes.byref(cin), ctypes.byref(cout), int(num_samples), int(interpolation), rot,
                                      ppost, dev, _stream_handle(stream))
    else:
        st = lib.lrp_reproject(ctypes.byref(cin), ctypes.byref(cout), int(num_samples), int(interpolation), rot, ppost,
                               0 if device is None else device)
    del keep
    _check(st)


def coverage(in_image, out_image, num_samples, rotation_matrix=None, out=None, mask_image=False, alpha_channel=-1, device=None,
             stream=None):
    """lrp_coverage_device (include/lrp.h "coverage"): how many of the num_samples^2 sub-samples of every output pixel the source
    image recorded — inside the source rectangle and, for a source that folds rays through x / -z, in front of the camera.
    Returns the (height, width) uint8 CUDA tensor of counts (`out` if given, else allocated).  mask_image: every channel of the
    count-0 pixels of out_image.data (a CUDA tensor) becomes +0.0; alpha_channel >= 0: that channel of every pixel becomes
    count / num_samples^2.  in_image.data is not read and may be None.  Asynchronous on `stream`."""
    import torch

    lib = _native.load()
    cin, cout = in_image.to_c(), out_image.to_c()
    keep, rot = _rotation_arg(rotation_matrix)
    if device is None:
        device = next((t.device.index for t in (out, out_image.data, in_image.data) if _is_torch(t) and t.is_cuda), 0)
    if out is None:
        out = torch.empty((out_image.height, out_image.width), dtype=torch.uint8, device=f"cuda:{device}")
    elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or out.numel() != out_image.height * out_image.width:
        raise _plane_error("out")
    st = lib.lrp_coverage_device(ctypes.byref(cin), ctypes.byref(cout), int(num_samples), rot, out.data_ptr(), int(bool(mask_image)),
                                 int(alpha_channel), device, _stream_handle(stream))
    del keep
    _check(st)
    return out


def compose(in_images, out_image, interpolation, rotation_matrices=None, mode=ComposeMode.FIRST, post=None, count=None, device=None,
            stream=None):
    """lrp_compose_device (include/lrp.h "compose"): up to COMPOSE_MAX_SOURCES source images of one source mode, each with its
    own lens parameters, size and rotation (rotation_matrices: one 3 x 3 matrix per source, or None), rendered into out_image by
    one launch — per output pixel only the sources that cover it (the coverage definition) are sampled, and `mode` says what
    becomes of them: the first one, their mean, or the mean weighted by the distance to the source's edge.  A pixel no source
    covers becomes +0.0.  Device tensors only; asynchronous on `stream`.  count: None, True (returns a new (height, width)
    uint8 CUDA tensor of the number of covering sources per pixel) or such a tensor to fill (returned)."""
    lib = _native.load()
    n = len(in_images)
    _check_planes(out_image.height, out_image.width, count=count)
    if not out_image.on_device() or not all(i.on_device() for i in in_images):
        raise ValueError("compose() takes device tensors only: the data of every input image and of the output must be a CUDA tensor")
    if device is None:
        device = out_image.data.device.index
    plane, = _alloc_planes(out_image.height, out_image.width, device, count)
    arr = (LrpImage * max(n, 1))(*[i.to_c() for i in in_images])
    cout = out_image.to_c()
    keep, rot = _rotations_arg(rotation_matrices, n)
    cpost, ppost = _post_arg(post)
    st = lib.lrp_compose_device(arr, n, rot, ctypes.byref(cout), int(interpolation), int(mode), ppost, _data_ptr(plane), device,
                                _stream_handle(stream))
    del keep
    _check(st)
    return plane


def compose_ss(in_images, out_image, num_samples, interpolation, rotation_matrices=None, mode=ComposeMode.FIRST, post=None, count=None,
               coverage=None, device=None, stream=None):
    """lrp_compose_ss_device (include/lrp.h "compose, supersampled"): compose() with num_samples x num_samples sub-samples per
    output pixel, by one launch — which sources cover a point is decided per sub-sample, every covered sub-sample is composed
    under `mode`, and the pixel is the mean of its covered sub-samples (+0.0 where none is).  Device tensors only; asynchronous
    on `stream`.  count / coverage: None, True (a new (height, width) uint8 CUDA tensor) or such a tensor to fill — count the
    number of sources that cover at least one sub-sample of the pixel, coverage the number of covered sub-samples, 0 ..
    num_samples^2.  Returns (count plane or None, coverage plane or None)."""
    lib = _native.load()
    n = len(in_images)
    _check_planes(out_image.height, out_image.width, count=count, coverage=coverage)
    if not out_image.on_device() or not all(i.on_device() for i in in_images):
        raise ValueError("compose_ss() takes device tensors only: the data of every input image and of the output must be a CUDA tensor")
    if device is None:
        device = out_image.data.device.index
    count, coverage = _alloc_planes(out_image.height, out_image.width, device, count, coverage)
    arr = (LrpImage * max(n, 1))(*[i.to_c() for i in in_images])
    cout = out_image.to_c()
    keep, rot = _rotations_arg(rotation_matrices, n)
    cpost, ppost = _post_arg(post)
    st = lib.lrp_compose_ss_device(arr, n, rot, ctypes.byref(cout), int(num_samples), int(interpolation), int(mode), ppost, _data_ptr(count),
                                   _data_ptr(coverage), device, _stream_handle(stream))
    del keep
    _check(st)
    return count, coverage


class CameraModel(enum.IntEnum):  # include/lrp.h lrp_camera_model
    BROWN = 0
    FISHEYE = 1


class Camera:
    """lrp_camera (include/lrp.h "compose, calibrated cameras"): one frame of a calibrated camera — fx, fy, cx, cy in pixels
    ((0, 0) is the centre of the top-left texel, as in OpenCV) and the distortion coefficients k: BROWN k1 k2 p1 p2 k3, FISHEYE
    (Kannala-Brandt) k1 k2 k3 k4.  data: a float32 CUDA tensor of width*height*channels elements, the channels being the
    output's.  limit: the largest r2 (BROWN) / theta (FISHEYE) the camera images; None asks lrp_camera_limit for the point
    where the polynomial stops increasing."""

    def __init__(self, model, width, height, data, fx, fy, cx, cy, k=(), limit=None):
        self.model = int(model)
        self.width = int(width)
        self.height = int(height)
        self.data = data
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
        k = list(k)
        if len(k) > 5:
            raise ValueError("a camera has at most 5 distortion coefficients")
        self.k = [float(np.float32(v)) for v in k + [0.0] * (5 - len(k))]
        self.limit = float(np.float32(limit)) if limit is not None else camera_limit(self)

    @classmethod
    def brown(cls, width, height, data, fx, fy, cx, cy, k=(0.0, 0.0, 0.0, 0.0, 0.0), limit=None):
        """Brown-Conrady: k = (k1, k2, p1, p2, k3), OpenCV's order."""
        return cls(CameraModel.BROWN, width, height, data, fx, fy, cx, cy, k, limit)

    @classmethod
    def fisheye(cls, width, height, data, fx, fy, cx, cy, k=(0.0, 0.0, 0.0, 0.0), limit=None):
        """Kannala-Brandt: k = (k1, k2, k3, k4), the order of OpenCV's fisheye module."""
        return cls(CameraModel.FISHEYE, width, height, data, fx, fy, cx, cy, k, limit)

    def on_device(self):
        return _is_torch(self.data) and self.data.is_cuda

    def to_c(self, channels=None, limit=None):
        """The lrp_camera; channels: the channel count the data tensor is checked against (None: data is not looked at and the
        pointer is NULL)."""
        c = _native.LrpCamera()
        c.model, c.width, c.height = self.model, self.width, self.height
        c.data = None
        if channels is not None and self.data is not None:
            import torch

            d = self.data
            if not _is_torch(d) or d.dtype != torch.float32 or not d.is_contiguous() or d.numel() != self.width * self.height * int(channels):
                raise ValueError("camera tensor must be contiguous float32 with width*height*channels elements")
            c.data = d.data_ptr()
        c.fx, c.fy, c.cx, c.cy = self.fx, self.fy, self.cx, self.cy
        for i in range(5):
            c.k[i] = self.k[i]
        c.limit = self.limit if limit is None else limit
        return c


def camera_limit(camera):
    """lrp_camera_limit (host only): the largest r2 (BROWN; inf when the radial polynomial increases up to r = 16) or theta
    (FISHEYE; at most pi) up to which the camera's distortion polynomial still increases — beyond it rays fold back into the
    frame as ghosts."""
    c = camera.to_c(limit=0.0)
    out = ctypes.c_float()
    _check(_native.load().lrp_camera_limit(ctypes.byref(c), ctypes.byref(out)))
    return float(out.value)


def compose_cameras(cameras, out_image, num_samples, interpolation, rotation_matrices=None, mode=ComposeMode.FIRST, post=None,
                    count=None, coverage=None, device=None, stream=None, gains=None):
    """lrp_compose_cameras_device (include/lrp.h "compose, calibrated cameras"): compose_ss() whose sources are frames of
    calibrated cameras (Camera; the models may be mixed), by one launch; a single camera into a rectilinear out_image
    undistorts it.  Device tensors only; asynchronous on `stream`.  count / coverage and the return value: as compose_ss().
    gains: one factor per camera on its first min(channels, 3) channels (camera_gains()); anything but None takes
    lrp_compose_cameras_gain_device (include/lrp.h "exposure matching across a camera rig")."""
    lib = _native.load()
    n = len(cameras)
    _check_planes(out_image.height, out_image.width, count=count, coverage=coverage)
    if not out_image.on_device() or not all(c.on_device() for c in cameras):
        raise ValueError("compose_cameras() takes device tensors only: the data of every camera and of the output must be a CUDA tensor")
    if device is None:
        device = out_image.data.device.index
    count, coverage = _alloc_planes(out_image.height, out_image.width, device, count, coverage)
    arr = (_native.LrpCamera * max(n, 1))(*[c.to_c(out_image.channels) for c in cameras])
    cout = out_image.to_c()
    keep, rot = _rotations_arg(rotation_matrices, n)
    cpost, ppost = _post_arg(post)
    tail = (ctypes.byref(cout), int(num_samples), int(interpolation), int(mode), ppost, _data_ptr(count), _data_ptr(coverage), device,
            _stream_handle(stream))
    if gains is None:
        st = lib.lrp_compose_cameras_device(arr, n, rot, *tail)
    else:
        g, gains_ptr = _gains_arg(gains, n)
        st = lib.lrp_compose_cameras_gain_device(arr, n, rot, gains_ptr, *tail)
    del keep
    _check(st)
    return count, coverage


MULTIBAND_MAX_BANDS = 8
MULTIBAND_NO_CAMERA = 255


def multiband_scratch_bytes(width, height, channels, num_bands):
    """lrp_multiband_scratch_bytes (host only): the bytes of scratch compose_cameras_multiband() needs for an output of this
    size and channel count with num_bands bands."""
    out = ctypes.c_size_t()
    _check(_native.load().lrp_multiband_scratch_bytes(int(width), int(height), int(channels), int(num_bands), ctypes.byref(out)))
    return int(out.value)


def compose_cameras_multiband(cameras, out_image, interpolation, rotation_matrices=None, num_bands=5, gains=None, post=None, count=None,
                              label=None, scratch=None, device=None, stream=None):
    """lrp_compose_cameras_multiband_device (include/lrp.h "multi-band blending across a camera rig"): the frames of calibrated
    cameras blended over a Laplacian pyramid of num_bands bands — low frequencies over wide zones, high frequencies over narrow
    ones — under the seams of the largest feather weight; num_samples is 1, 1 .. 4 channels.  Device tensors only; asynchronous
    on `stream`.  gains: as compose_cameras().  scratch: a contiguous uint8 CUDA tensor of at least multiband_scratch_bytes(...)
    bytes aligned to 256, or None to allocate one.  count / label: True to allocate the plane, a uint8 CUDA tensor of
    height * width elements to fill, None to leave it out; the return value is the pair (count, label) — the number of cameras
    that cover each pixel, and the camera that wins it (MULTIBAND_NO_CAMERA where none does)."""
    lib = _native.load()
    n = len(cameras)
    _check_planes(out_image.height, out_image.width, count=count, label=label)
    if not out_image.on_device() or not all(c.on_device() for c in cameras):
        raise ValueError("compose_cameras_multiband() takes device tensors only: the data of every camera and of the output must be a CUDA tensor")
    if device is None:
        device = out_image.data.device.index
    count, label = _alloc_planes(out_image.height, out_image.width, device, count, label)
    scratch = _scratch_arg(scratch, out_image, num_bands, device)
    arr = (_native.LrpCamera * max(n, 1))(*[c.to_c(out_image.channels) for c in cameras])
    cout = out_image.to_c()
    keep, rot = _rotations_arg(rotation_matrices, n)
    g, gains_ptr = _gains_arg(gains, n)
    cpost, ppost = _post_arg(post)
    st = lib.lrp_compose_cameras_multiband_device(arr, n, rot, gains_ptr, ctypes.byref(cout), int(interpolation), int(num_bands), ppost,
                                                  _data_ptr(count), _data_ptr(label), scratch.data_ptr(), scratch.numel(), device,
                                                  _stream_handle(stream))
    del keep
    _check(st)
    return count, label


def camera_overlap(cameras, out_image, rotation_matrices=None, lo=0.02, hi=0.98, stats=None, device=None, stream=None):
    """lrp_camera_overlap_device (include/lrp.h "exposure matching across a camera rig"): the statistic of the cameras' pairwise
    overlaps in out_image's geometry (its lens, size and channel count; its data is not looked at), by one launch: an int64 CUDA
    tensor of shape (8, 8, 2) with [i, j] = (N_ij, S_ij) — the number of output pixels at which cameras i and j both have a
    luminance inside [lo, hi], and the sum of camera i's luminance over them in units of 1 / 65536.  stats: a tensor to write
    into (every word is overwritten), or None to allocate one.  Asynchronous on `stream`."""
    lib = _native.load()
    n = len(cameras)
    if not all(c.on_device() for c in cameras):
        raise ValueError("camera_overlap() takes device tensors only: the data of every camera must be a CUDA tensor")
    if device is None:
        device = cameras[0].data.device.index if n else 0
    _check_stats(stats)
    stats = _stats_arg(stats, device)
    arr = (_native.LrpCamera * max(n, 1))(*[c.to_c(out_image.channels) for c in cameras])
    cout = Image(out_image.lens, out_image.width, out_image.height, out_image.channels, None).to_c()
    keep, rot = _rotations_arg(rotation_matrices, n)
    st = lib.lrp_camera_overlap_device(arr, n, rot, ctypes.byref(cout), float(lo), float(hi), stats.data_ptr(), device, _stream_handle(stream))
    del keep
    _check(st)
    return stats


def camera_gains(stats, n, sigma_n=10 / 255, sigma_g=0.1):
    """lrp_camera_gains (host only): Brown and Lowe's gain compensation on the table of camera_overlap() — a tensor or an array
    of 8 * 8 * 2 integers, copied to the host — for its first n cameras: float32[n], the factor per camera that equalises the
    overlaps' mean luminances under a prior of unit gain.  A camera without a valid pixel gets 1.0."""
    host = stats.cpu().numpy() if _is_torch(stats) else np.asarray(stats)
    table = np.ascontiguousarray(host.astype(np.uint64, copy=False).reshape(-1))
    if table.size != 128:
        raise ValueError("stats must hold 8*8*2 integers")
    gains = np.empty(max(int(n), 1), dtype=np.float32)
    _check(_native.load().lrp_camera_gains(table.ctypes.data, int(n), float(sigma_n), float(sigma_g), gains.ctypes.data))
    return gains[: int(n)]


def camera_view(cameras, target, out, num_samples, interpolation, rotation_matrices=None, mode=ComposeMode.FIRST, post=None, count=None,
                coverage=None, device=None, stream=None):
    """lrp_camera_view_device (include/lrp.h "calibrated camera as the target"): compose_cameras() into the frame of another
    calibrated camera — a new camera matrix, camera-to-camera remapping, re-distortion.  target: a Camera whose data is
    ignored; out: a float32 CUDA tensor of target.height * target.width * channels elements, channels being every camera's.
    Pixels of the target for which its polynomial has no ray are +0.0 with coverage 0.  Device tensors only; asynchronous on
    `stream`.  count / coverage and the return value: as compose_cameras()."""
    import torch

    lib = _native.load()
    n = len(cameras)
    px = target.width * target.height
    if (not _is_torch(out) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or px <= 0 or out.numel() == 0
            or out.numel() % px != 0):
        raise ValueError("out must be a contiguous float32 CUDA tensor with height*width*channels elements")
    channels = out.numel() // px
    _check_planes(target.height, target.width, count=count, coverage=coverage)
    if not all(c.on_device() for c in cameras):
        raise ValueError("camera_view() takes device tensors only: the data of every camera must be a CUDA tensor")
    if device is None:
        device = out.device.index
    count, coverage = _alloc_planes(target.height, target.width, device, count, coverage)
    arr = (_native.LrpCamera * max(n, 1))(*[c.to_c(channels) for c in cameras])
    ctarget = target.to_c()
    keep, rot = _rotations_arg(rotation_matrices, n)
    cpost, ppost = _post_arg(post)
    st = lib.lrp_camera_view_device(arr, n, rot, ctypes.byref(ctarget), out.data_ptr(), channels, int(num_samples), int(interpolation),
                                    int(mode), ppost, _data_ptr(count), _data_ptr(coverage), device, _stream_handle(stream))
    del keep
    _check(st)
    return count, coverage


def camera_unproject(camera, uv):
    """lrp_camera_unproject (host only): the rays of the pixel positions uv (N, 2) of a calibrated camera — the inverse the
    camera_view() kernel evaluates, with its bits; the library's undistortPoints.  Returns (rays (N, 3) float32, has_ray (N,)
    bool); a BROWN ray is (X, Y, -1), a FISHEYE ray has unit length."""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    n = uv.shape[0]
    rays = np.empty((n, 3), dtype=np.float32)
    has_ray = np.empty(n, dtype=np.uint8)
    c = camera.to_c()
    _check(_native.load().lrp_camera_unproject(ctypes.byref(c), uv.ctypes.data, n, rays.ctypes.data, has_ray.ctypes.data))
    return rays, has_ray.astype(bool)


def reproject_multi(in_image, out_images, num_samples, interpolation, rotation_matrices=None, post=None, device=None,
                    stream=None):
    """One resident source, several target lenses / rotations (device tensors only)."""
    lib = _native.load()
    cin = in_image.to_c()
    arr = (LrpImage * len(out_images))(*[o.to_c() for o in out_images])
    keep, rot = _rotations_arg(rotation_matrices, len(out_images))
    cpost, ppost = _post_arg(post)
    dev = in_image.data.device.index if device is None else device
    st = lib.lrp_reproject_multi_device(ctypes.byref(cin), arr, len(out_images), int(num_samples), int(interpolation), rot, ppost, dev,
                                        _stream_handle(stream))
    del keep
    _check(st)


def reproject_rows(in_image, out_image, num_samples, interpolation, row_first, row_count, rotation_matrix=None, post=None,
                   device=None, stream=None):
    """lrp_reproject_rows_device: rows [row_first, row_first + row_count) of the output only (device tensors)."""
    lib = _native.load()
    cin, cout = in_image.to_c(), out_image.to_c()
    keep, rot = _rotation_arg(rotation_matrix)
    cpost, ppost = _post_arg(post)
    dev = in_image.data.device.index if device is None else device
    st = lib.lrp_reproject_rows_device(ctypes.byref(cin), ctypes.byref(cout), int(num_samples), int(interpolation), rot, ppost,
                                       int(row_first), int(row_count), dev, _stream_handle(stream))
    del keep
    _check(st)


def reproject_multi_gpu(in_image, out_images, num_samples, interpolation, rotation_matrices=None, post=None, devices=(0,)):
    """lrp_reproject_multi: one host source, several host outputs, row bands of every output on every listed GPU."""
    lib = _native.load()
    cin = in_image.to_c()
    arr = (LrpImage * len(out_images))(*[o.to_c() for o in out_images])
    keep, rot = _rotations_arg(rotation_matrices, len(out_images))
    cpost, ppost = _post_arg(post)
    devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
    st = lib.lrp_reproject_multi(ctypes.byref(cin), arr, len(out_images), int(num_samples), int(interpolation), rot, ppost, devs,
                                 len(devices))
    del keep
    _check(st)


def reproject_batch(in_images, out_images, num_samples, interpolation, rotation_matrix=None, post=None, device=None,
                    stream=None):
    """n images of one geometry (same sizes, channels, lenses), device tensors only: one kernel
    launch per 16 images (lrp_reproject_batch_device); results equal n reproject() calls."""
    lib = _native.load()
    if len(in_images) != len(out_images):
        raise ValueError("in_images and out_images must have the same length")
    if not in_images:
        return
    ins = (LrpImage * len(in_images))(*[i.to_c() for i in in_images])
    outs = (LrpImage * len(out_images))(*[o.to_c() for o in out_images])
    keep, rot = _rotation_arg(rotation_matrix)
    cpost, ppost = _post_arg(post)
    dev = in_images[0].data.device.index if device is None else device
    st = lib.lrp_reproject_batch_device(ins, outs, len(in_images), int(num_samples), int(interpolation), rot, ppost, dev,
                                        _stream_handle(stream))
    del keep
    _check(st)


class PreparedBatch:
    """The arguments of one lrp_reproject_batch_device call, marshalled once: launch() is then a single
    foreign call (a directory of frames of one geometry is launched many times with the same descriptors)."""

    def __init__(self, in_images, out_images, num_samples, interpolation, rotation_matrix=None, post=None, device=None):
        if len(in_images) != len(out_images) or not in_images:
            raise ValueError("in_images and out_images must be non-empty and of equal length")
        self._lib = _native.load()
        self._keep = (list(in_images), list(out_images))
        self._n = len(in_images)
        self._ins = (LrpImage * self._n)(*[i.to_c() for i in in_images])
        self._outs = (LrpImage * self._n)(*[o.to_c() for o in out_images])
        self._rot_keep, self._rot = _rotation_arg(rotation_matrix)
        self._post = LrpPost(float(post[0]), float(post[1])) if post is not None else None
        self._args = (int(num_samples), int(interpolation))
        self._dev = in_images[0].data.device.index if device is None else device

    def launch(self, stream=None):
        _check(self._lib.lrp_reproject_batch_device(self._ins, self._outs, self._n, self._args[0], self._args[1], self._rot,
                                                    ctypes.byref(self._post) if self._post is not None else None, self._dev,
                                                    _stream_handle(stream)))


def post_process(image, exposure, reinhard, device=None, stream=None):
    """reproject::post_process (src/reproject.cpp:421-437), in place."""
    lib = _native.load()
    c = image.to_c()
    if image.on_device():
        dev = image.data.device.index if device is None else device
        st = lib.lrp_post_process_device(ctypes.byref(c), exposure, reinhard, dev, _stream_handle(stream))
    else:
        st = lib.lrp_post_process(ctypes.byref(c), exposure, reinhard, 0 if device is None else device)
    _check(st)


def test_conversion_math():
    """reproject::test_conversion_math (src/reproject.cpp:467): an empty function in the reference."""
    return None


class BatchContext:
    """lrp_context: n_streams streams on one device for batches of independent
    host images (the reference's one-file-per-pool-thread path, src/main.cpp:538-622)."""

    def __init__(self, device=0, n_streams=3):
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        _check(self._lib.lrp_context_create(ctypes.byref(self._h), device, n_streams))
        self._keep = []

    def submit(self, in_image, out_image, num_samples, interpolation, rotation_matrix=None, post=None):
        cin, cout = in_image.to_c(), out_image.to_c()
        keep, rot = _rotation_arg(rotation_matrix)
        cpost, ppost = _post_arg(post)
        self._keep.append((in_image, out_image, keep))
        _check(self._lib.lrp_context_submit(self._h, ctypes.byref(cin), ctypes.byref(cout), int(num_samples),
                                            int(interpolation), rot, ppost))

    def submit_packed(self, in_image, in_format, in_data, out_image, out_format, out_data, out_fill, num_samples,
                      interpolation, rotation_matrix=None, post=None):
        """lrp_context_submit_packed: `in_data` / `out_data` are C-contiguous numpy arrays of shape
        (height, width, packed_channels) in the file formats (float16 / uint8 / float32); the images
        describe the float geometry the kernels see.  Returns a ticket for wait_ticket()."""
        cin, cout = in_image.to_c(), out_image.to_c()
        cin.data = in_data.ctypes.data
        cout.data = out_data.ctypes.data
        keep, rot = _rotation_arg(rotation_matrix)
        cpost, ppost = _post_arg(post)
        ticket = ctypes.c_int(-1)
        self._keep.append((in_data, out_data, keep))
        _check(self._lib.lrp_context_submit_packed(self._h, ctypes.byref(cin), int(in_format), int(in_data.shape[-1]),
                                                   ctypes.byref(cout), int(out_format), int(out_data.shape[-1]),
                                                   int(out_fill), int(num_samples), int(interpolation), rot, ppost,
                                                   ctypes.byref(ticket)))
        return ticket.value

    def set_outside(self, mask_image=False, alpha_channel=-1):
        """lrp_context_set_outside: for the images submitted from now on, the coverage kernel follows the reprojection — the
        pixels the source cannot see become +0.0 (mask_image) and / or a channel receives the coverage fraction (alpha_channel).
        (False, -1) switches it off."""
        _check(self._lib.lrp_context_set_outside(self._h, int(bool(mask_image)), int(alpha_channel)))

    def wait_ticket(self, ticket):
        _check(self._lib.lrp_context_wait_ticket(self._h, int(ticket)))

    def wait(self):
        st = self._lib.lrp_context_wait(self._h)
        self._keep.clear()
        _check(st)

    def close(self):
        if self._h:
            self._lib.lrp_context_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def synth_fill(tensor, width, height, channels, seed, depth_channel=-1, stream=None):
    """Fill a float32 CUDA tensor with the synthetic frame of SURVEY.md §8d."""
    lib = _native.load()
    _check(lib.lrp_synth_fill_device(tensor.data_ptr(), width, height, channels, seed & 0xFFFFFFFF, depth_channel,
                                     tensor.device.index, _stream_handle(stream)))


def math_eval(func, a, b=None, stream=None):
    """Run one device math routine element-wise on CUDA tensors (tests)."""
    import torch

    lib = _native.load()
    out = torch.empty_like(a)
    _check(lib.lrp_math_eval_device(int(func), a.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(),
                                    a.numel(), a.device.index, _stream_handle(stream)))
    return out


def checksums(tensors, stream=None):
    """Order-independent 64-bit checksums (lrp_checksum_device) of float32 CUDA tensors, one
    device pass per tensor and a single read-back: a list of Python ints."""
    import torch

    lib = _native.load()
    if not tensors:
        return []
    dev = tensors[0].device
    out = torch.zeros(len(tensors), dtype=torch.int64, device=dev)
    for i, t in enumerate(tensors):
        _check(lib.lrp_checksum_device(t.data_ptr(), t.numel(), out.data_ptr() + 8 * i, dev.index, _stream_handle(stream)))
    return [int(v) & 0xFFFFFFFFFFFFFFFF for v in out.cpu().tolist()]


def checksum_host(array):
    """The same checksum evaluated with numpy on a host array (tests)."""
    bits = np.ascontiguousarray(array, dtype=np.float32).reshape(-1).view(np.uint32)
    idx = np.arange(bits.size, dtype=np.uint32)

    def mix32(seed, index):
        with np.errstate(over="ignore"):
            h = index * np.uint32(0x9E3779B9) + seed
            h ^= h >> np.uint32(16)
            h *= np.uint32(0x7FEB352D)
            h ^= h >> np.uint32(15)
            h *= np.uint32(0x846CA68B)
            h ^= h >> np.uint32(16)
        return h

    with np.errstate(over="ignore"):
        lo = mix32(bits, idx).astype(np.uint64)
        hi = mix32(bits ^ np.uint32(0xA5A5A5A5), idx * np.uint32(2) + np.uint32(0x7F4A7C15)).astype(np.uint64)
        return int(np.sum((hi << np.uint64(32)) | lo, dtype=np.uint64))


class PixelFormat(enum.IntEnum):  # include/lrp.h lrp_pixel_format
    F32 = 0
    F16 = 1
    U8_GAMMA = 2


def decode_pixels(src, src_format, dst, stream=None):
    """lrp_decode_pixels_device: `src` a CUDA tensor (..., src_channels) of uint8 / int16 (half bits) / float16 /
    float32 samples, `dst` a float32 CUDA tensor (..., dst_channels) with the same number of pixels."""
    lib = _native.load()
    n = dst.numel() // dst.shape[-1]
    _check(lib.lrp_decode_pixels_device(src.data_ptr(), int(src_format), int(src.shape[-1]), dst.data_ptr(), int(dst.shape[-1]),
                                        n, dst.device.index, _stream_handle(stream)))


def encode_pixels(src, dst, dst_format, fill=0, stream=None):
    """lrp_encode_pixels_device: float32 CUDA tensor (..., C) -> `dst` (..., dst_channels) in `dst_format`."""
    lib = _native.load()
    n = src.numel() // src.shape[-1]
    _check(lib.lrp_encode_pixels_device(src.data_ptr(), int(src.shape[-1]), dst.data_ptr(), int(dst_format), int(dst.shape[-1]),
                                        int(fill), n, src.device.index, _stream_handle(stream)))


# the kernels address a packed tensor by its format's sample size: a tensor of narrower elements would be read or written past
# its end (an unknown format is left to the library's own LRP_ERR_BAD_ARG)
_SAMPLE_BYTES = {int(PixelFormat.F32): 4, int(PixelFormat.F16): 2, int(PixelFormat.U8_GAMMA): 1}


def _packed_tensor_check(who, tensors):
    """The three checks of every packed tensor of the call who(), tensor by tensor: on the device and contiguous, elements of the
    format's sample size, height * width pixels of shape[-1] samples.  tensors: (name, tensor, format, the image or camera that
    has the width and the height) each.  One call per list, not per tensor: the mirrors' time shows in the small launches."""
    for name, t, fmt, sized in tensors:
        if not _is_torch(t) or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{who}() takes device tensors only: {name} must be a contiguous CUDA tensor")
        fmt = int(fmt)
        if fmt in _SAMPLE_BYTES and t.element_size() != _SAMPLE_BYTES[fmt]:
            raise ValueError(f"{name}: elements of {t.element_size()} bytes ({t.dtype}) for a format of {_SAMPLE_BYTES[fmt]}-byte samples")
        if t.dim() < 1 or t.numel() != sized.width * sized.height * t.shape[-1]:
            raise ValueError(f"{name}: packed tensors must hold height*width pixels of shape[-1] samples")


def _packed_image(image, tensor):
    """The lrp_image of a packed call: image's lens, size and channel count around tensor's pointer (image.data is not looked at)."""
    c = LrpImage()
    c.lens = image.lens.to_c()
    c.width, c.height, c.channels = image.width, image.height, image.channels
    c.data = tensor.data_ptr()
    c.data_layout = image.data_layout
    return c


def reproject_packed(in_image, in_format, in_data, out_image, out_format, out_data, out_fill, num_samples, interpolation,
                     rotation_matrix=None, post=None, device=None, stream=None):
    """lrp_reproject_packed_device (include/lrp.h "packed pixels"): BatchContext.submit_packed's decode, reproject and encode as
    one launch on the device.  `in_data` / `out_data` are contiguous CUDA tensors of shape (height, width, packed_channels) in
    the file formats — uint8, int16 (half bits) / float16, float32 (output only), as decode_pixels takes them; the images
    describe the float geometry (their own data is not looked at).  The output bytes are those of decode_pixels -> reproject
    -> encode_pixels.  Asynchronous on `stream` (default: torch's current stream)."""
    lib = _native.load()
    # _packed_tensor_check's checks in this call's own order and wording — every tensor's first check, then every tensor's second,
    # then the third without the tensor's name — which it has had since it was the only packed call
    for name, t in (("in_data", in_data), ("out_data", out_data)):
        if not _is_torch(t) or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"reproject_packed() takes device tensors only: {name} must be a contiguous CUDA tensor")
    for name, t, fmt in (("in_data", in_data, int(in_format)), ("out_data", out_data, int(out_format))):
        if fmt in _SAMPLE_BYTES and t.element_size() != _SAMPLE_BYTES[fmt]:
            raise ValueError(f"{name}: elements of {t.element_size()} bytes ({t.dtype}) for a format of {_SAMPLE_BYTES[fmt]}-byte samples")
    if (in_data.numel() != in_image.width * in_image.height * in_data.shape[-1]
            or out_data.numel() != out_image.width * out_image.height * out_data.shape[-1]):
        raise ValueError("packed tensors must hold height*width pixels of shape[-1] samples")
    cin, cout = _packed_image(in_image, in_data), _packed_image(out_image, out_data)
    keep, rot = _rotation_arg(rotation_matrix)
    cpost, ppost = _post_arg(post)
    dev = in_data.device.index if device is None else device
    st = lib.lrp_reproject_packed_device(ctypes.byref(cin), int(in_format), int(in_data.shape[-1]), ctypes.byref(cout), int(out_format),
                                         int(out_data.shape[-1]), int(out_fill), int(num_samples), int(interpolation), rot, ppost, dev,
                                         _stream_handle(stream))
    del keep
    _check(st)


def compose_packed(in_images, in_format, in_datas, out_image, out_format, out_data, out_fill, interpolation, rotation_matrices=None,
                   mode=ComposeMode.FIRST, post=None, count=None, device=None, stream=None):
    """lrp_compose_packed_device (include/lrp.h "compose, packed pixels"): compose() on sources and an output in their file
    formats, as one launch — the bytes of decode_pixels per source -> compose -> encode_pixels without the float32 staging
    images.  `in_datas` (one per source, all in `in_format` and of one packed channel count) and `out_data` are contiguous CUDA
    tensors of shape (height, width, packed_channels) as reproject_packed() takes them; the images describe the float geometry
    (their own data is not looked at).  rotation_matrices, mode, post and count (None, True or a tensor to fill; returned) as in
    compose().  Asynchronous on `stream` (default: torch's current stream)."""
    lib = _native.load()
    n = len(in_images)
    in_datas = list(in_datas)
    if len(in_datas) != n:
        raise ValueError(f"compose_packed(): {n} source images but {len(in_datas)} packed tensors")
    named = [(f"in_datas[{i}]", t, int(in_format), im) for i, (t, im) in enumerate(zip(in_datas, in_images))]
    named.append(("out_data", out_data, int(out_format), out_image))
    _packed_tensor_check("compose_packed", named)
    if any(t.shape[-1] != in_datas[0].shape[-1] for t in in_datas[1:]):
        raise ValueError("compose_packed(): every source must have the same number of packed channels")
    _check_planes(out_image.height, out_image.width, count=count)
    if device is None:
        device = out_data.device.index
    plane, = _alloc_planes(out_image.height, out_image.width, device, count)
    arr = (LrpImage * max(n, 1))(*[_packed_image(im, t) for im, t in zip(in_images, in_datas)])
    cout = _packed_image(out_image, out_data)
    keep, rot = _rotations_arg(rotation_matrices, n)
    cpost, ppost = _post_arg(post)
    st = lib.lrp_compose_packed_device(arr, n, int(in_format), int(in_datas[0].shape[-1]) if n else 0, rot, ctypes.byref(cout), int(out_format),
                                       int(out_data.shape[-1]), int(out_fill), int(interpolation), int(mode), ppost, _data_ptr(plane), device,
                                       _stream_handle(stream))
    del keep
    _check(st)
    return plane


def _packed_camera_check(who, cameras, in_format, in_datas):
    """reproject_packed()'s checks of every packed frame against its camera's size and the format's sample size; returns the
    packed channel count.  No pointer is taken."""
    n = len(cameras)
    if len(in_datas) != n:
        raise ValueError(f"{who}(): {n} cameras but {len(in_datas)} packed tensors")
    fmt = int(in_format)
    _packed_tensor_check(who, ((f"in_datas[{i}]", t, fmt, cam) for i, (t, cam) in enumerate(zip(in_datas, cameras))))
    if any(t.shape[-1] != in_datas[0].shape[-1] for t in in_datas[1:]):
        raise ValueError(f"{who}(): every camera must have the same number of packed channels")
    return int(in_datas[0].shape[-1]) if n else 0


def _packed_camera_array(cameras, in_datas):
    """The lrp_camera array of a packed camera call: camera i's pointer is in_datas[i]'s (after _packed_camera_check)."""
    arr = (_native.LrpCamera * max(len(cameras), 1))(*[c.to_c() for c in cameras])
    for i, t in enumerate(in_datas):
        arr[i].data = t.data_ptr()
    return arr


def compose_cameras_packed(cameras, in_format, in_datas, out_image, out_format, out_data, out_fill, num_samples, interpolation,
                           rotation_matrices=None, mode=ComposeMode.FIRST, post=None, count=None, coverage=None, device=None, stream=None,
                           gains=None):
    """lrp_compose_cameras_packed_device (include/lrp.h "calibrated cameras, packed pixels"): compose_cameras() on frames and an
    output in their file formats, as one launch — the bytes of decode_pixels per camera -> compose_cameras(gains=) ->
    encode_pixels without the float32 staging images.  `in_datas` (one per camera, all in `in_format` and of one packed channel
    count) and `out_data` are contiguous CUDA tensors of shape (height, width, packed_channels) as reproject_packed() takes them;
    the cameras give the geometry (their own data is not looked at) and out_image the lens, the size and the channel count C.
    rotation_matrices, mode, post, count / coverage (None, True or a tensor to fill; both returned) and gains as in
    compose_cameras().  Asynchronous on `stream` (default: torch's current stream)."""
    lib = _native.load()
    n = len(cameras)
    in_datas = list(in_datas)
    in_pch = _packed_camera_check("compose_cameras_packed", cameras, in_format, in_datas)
    _packed_tensor_check("compose_cameras_packed", (("out_data", out_data, out_format, out_image),))
    _check_planes(out_image.height, out_image.width, count=count, coverage=coverage)
    g, gains_ptr = _gains_arg(gains, n)
    if device is None:
        device = out_data.device.index
    count, coverage = _alloc_planes(out_image.height, out_image.width, device, count, coverage)
    arr = _packed_camera_array(cameras, in_datas)
    cout = _packed_image(out_image, out_data)
    keep, rot = _rotations_arg(rotation_matrices, n)
    cpost, ppost = _post_arg(post)
    st = lib.lrp_compose_cameras_packed_device(arr, n, int(in_format), in_pch, rot, gains_ptr, ctypes.byref(cout), int(out_format),
                                               int(out_data.shape[-1]), int(out_fill), int(num_samples), int(interpolation), int(mode), ppost,
                                               _data_ptr(count), _data_ptr(coverage), device, _stream_handle(stream))
    del keep, g
    _check(st)
    return count, coverage


def camera_overlap_packed(cameras, in_format, in_datas, out_image, rotation_matrices=None, lo=0.02, hi=0.98, stats=None, device=None,
                          stream=None):
    """lrp_camera_overlap_packed_device (include/lrp.h "calibrated cameras, packed pixels"): camera_overlap() on frames in their
    file formats, as one launch — the table of decode_pixels per camera -> camera_overlap(), word for word, without the float32
    frames.  `in_datas` as in compose_cameras_packed(); out_image gives the lens, the size and the channel count C (its data is
    not looked at).  The table feeds camera_gains() unchanged.  Asynchronous on `stream`."""
    lib = _native.load()
    n = len(cameras)
    in_datas = list(in_datas)
    in_pch = _packed_camera_check("camera_overlap_packed", cameras, in_format, in_datas)
    _check_stats(stats)  # (before the device is looked for, as the planes of the compose calls are)
    if device is None:
        device = in_datas[0].device.index if n else 0
    stats = _stats_arg(stats, device)
    arr = _packed_camera_array(cameras, in_datas)
    cout = Image(out_image.lens, out_image.width, out_image.height, out_image.channels, None).to_c()
    keep, rot = _rotations_arg(rotation_matrices, n)
    st = lib.lrp_camera_overlap_packed_device(arr, n, int(in_format), in_pch, rot, ctypes.byref(cout), float(lo), float(hi), stats.data_ptr(),
                                              device, _stream_handle(stream))
    del keep
    _check(st)
    return stats


def compose_cameras_multiband_packed(cameras, in_format, in_datas, out_image, out_format, out_data, out_fill, interpolation,
                                     rotation_matrices=None, num_bands=5, gains=None, post=None, count=None, label=None, scratch=None,
                                     device=None, stream=None):
    """lrp_compose_cameras_multiband_packed_device (include/lrp.h "multi-band blending, packed pixels"): compose_cameras_multiband()
    on frames and an output in their file formats — the bytes of decode_pixels per camera -> compose_cameras_multiband() ->
    encode_pixels without the float32 frames and the float32 panorama.  `in_datas`, `out_data`, `out_fill` and out_image as in
    compose_cameras_packed(); rotation_matrices, num_bands, gains, post, count / label (None, True or a tensor to fill) and scratch
    (None allocates it; multiband_scratch_bytes() states its size) as in compose_cameras_multiband().  Returns (count, label).
    Asynchronous on `stream` (default: torch's current stream)."""
    lib = _native.load()
    n = len(cameras)
    in_datas = list(in_datas)
    in_pch = _packed_camera_check("compose_cameras_multiband_packed", cameras, in_format, in_datas)
    _packed_tensor_check("compose_cameras_multiband_packed", (("out_data", out_data, out_format, out_image),))
    _check_planes(out_image.height, out_image.width, count=count, label=label)
    g, gains_ptr = _gains_arg(gains, n)
    if device is None:
        device = out_data.device.index
    count, label = _alloc_planes(out_image.height, out_image.width, device, count, label)
    scratch = _scratch_arg(scratch, out_image, num_bands, device)
    arr = _packed_camera_array(cameras, in_datas)
    cout = _packed_image(out_image, out_data)
    keep, rot = _rotations_arg(rotation_matrices, n)
    cpost, ppost = _post_arg(post)
    st = lib.lrp_compose_cameras_multiband_packed_device(
        arr, n, int(in_format), in_pch, rot, gains_ptr, ctypes.byref(cout), int(out_format), int(out_data.shape[-1]), int(out_fill),
        int(interpolation), int(num_bands), ppost, _data_ptr(count), _data_ptr(label), scratch.data_ptr(), scratch.numel(), device,
        _stream_handle(stream))
    del keep, g
    _check(st)
    return count, label


def pixel_tables():
    """(decode[256], threshold[256]) of LRP_PIXEL_U8_GAMMA as the host's powf made them."""
    dec = (ctypes.c_float * 256)()
    thr = (ctypes.c_float * 256)()
    _native.load().lrp_pixel_tables(dec, thr)
    return np.frombuffer(dec, dtype=np.float32).copy(), np.frombuffer(thr, dtype=np.float32).copy()
