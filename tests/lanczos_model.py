"""ctypes binding of tests/native/lanczos_model.cpp — the CPU model of the Lanczos-3 sampler (include/lrp.h "Lanczos-3").  The
source coordinates come from tests/coverage_model.py (coverage(..., detail=True): all five lenses, every sub-sample in the
loop's order), so no lens formula is restated here.  Test infrastructure; built by __graft_entry__.build()."""
import ctypes
import math
import os

import numpy as np

import coverage_model
import oracle_binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "_build", "liblanczos_model.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        L.lzm_weights.restype = None
        L.lzm_weights.argtypes = [ctypes.c_float, ctypes.c_void_p]
        L.lzm_weights_n.restype = None
        L.lzm_weights_n.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        L.lzm_sample.restype = None
        L.lzm_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                 ctypes.c_void_p]
        L.lzm_render.restype = ctypes.c_int
        L.lzm_render.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong,
                                 ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
        _lib = L
    return _lib


def weights(f):
    """The six axis weights of the fraction(s) f: (6,) for a scalar, (n, 6) for an array."""
    L = lib()
    fs = np.atleast_1d(np.asarray(f, dtype=np.float32))
    out = np.empty((fs.size, 6), dtype=np.float32)
    if fs.size == 1:
        L.lzm_weights(float(fs[0]), out.ctypes.data)
    else:
        fs = np.ascontiguousarray(fs)
        L.lzm_weights_n(fs.ctypes.data, fs.size, out.ctypes.data)
    return out[0] if np.ndim(f) == 0 else out


def sample(src, loop, sx, sy):
    """One sample of src (H, W, C) at (sx, sy): (C,) float32."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    h, w, c = src.shape
    out = np.empty(c, dtype=np.float32)
    lib().lzm_sample(src.ctypes.data, w, h, c, int(bool(loop)), float(np.float32(sx)), float(np.float32(sy)), out.ctypes.data)
    return out


def render_coords(src, loop, sxy):
    """The accumulate loop over sxy (..., n2, 2) float32 — acc = 0; acc += sample; acc * (1.0f / n2) — : (..., C)."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    sxy = np.ascontiguousarray(sxy, dtype=np.float32)
    h, w, c = src.shape
    n2 = sxy.shape[-2]
    n_pixels = sxy.size // (2 * n2)
    out = np.empty(sxy.shape[:-2] + (c,), dtype=np.float32)
    normalize = np.float32(1.0) / np.float32(n2)
    rc = lib().lzm_render(src.ctypes.data, w, h, c, int(bool(loop)), sxy.ctypes.data, n_pixels, n2, float(normalize), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"lzm_render: {rc}")
    return out


def source_wraps(lens):
    """LoopHorizontally of the reference (src/reproject.cpp:386-394): a float span compared in double with a float threshold."""
    if int(lens.type) != 4:
        return False
    span = np.float32(lens.params[3]) - np.float32(lens.params[2])
    return abs(float(span) - 2.0 * math.pi) < float(np.float32(1e-5))


def coords(in_lens, in_w, in_h, out_lens, out_w, out_h, num_samples, rotation=None):
    """(out_h, out_w, n * n, 2) float32: the coordinates every sampler of that call receives."""
    return coverage_model.coverage(in_lens, in_w, in_h, out_lens, out_w, out_h, num_samples, rotation, detail=True)[1]


def reproject(in_lens, src, out_lens, out_w, out_h, num_samples, rotation=None, post=None):
    """Model of reproject(..., interpolation=LANCZOS3): src (H, W, C) float32 -> (out_h, out_w, C)."""
    h, w, _ = src.shape
    out = render_coords(src, source_wraps(in_lens), coords(in_lens, w, h, out_lens, out_w, out_h, num_samples, rotation))
    if post is not None:
        oracle_binding.post_process(out, float(post[0]), float(post[1]))
    return out
