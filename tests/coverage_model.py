"""ctypes binding of tests/native/coverage_model.c — the CPU model of the coverage planes (include/lrp.h "coverage"): the
stereographic model's loop, samplers and five lenses plus coverage(), which applies the definition to the coordinates and rays
of the very lens functions the render loop calls.  Test infrastructure; built by __graft_entry__.build()."""
import ctypes
import os

import numpy as np

import oracle_binding as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "_build", "libcoverage_model.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        I = oracle.OImage  # same layout as cvm_image
        L.cvm_reproject.restype = ctypes.c_int
        L.cvm_reproject.argtypes = [P(I), P(I), ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.cvm_post_process.restype = None
        L.cvm_post_process.argtypes = [P(I), ctypes.c_float, ctypes.c_float]
        L.cvm_coverage.restype = ctypes.c_int
        L.cvm_coverage.argtypes = [P(I), P(I), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def reproject(in_lens, src, out_lens, out_w, out_h, num_samples, interpolation, rotation=None, post=None):
    """Model reproject(): src (H, W, C) float32 -> (out_h, out_w, C); post = (exposure, reinhard) applies post_process."""
    L = lib()
    src = np.ascontiguousarray(src, dtype=np.float32)
    h, w, c = src.shape
    out = np.full((out_h, out_w, c), np.float32(-12345.0), dtype=np.float32)
    cin = oracle._image(in_lens, w, h, c, src)
    cout = oracle._image(out_lens, out_w, out_h, c, out)
    keep, rp = oracle._rot(rotation)
    rc = L.cvm_reproject(ctypes.byref(cin), ctypes.byref(cout), int(num_samples), int(interpolation), rp)
    if rc != 0:
        raise ValueError(f"cvm_reproject: {rc}")
    if post is not None:
        L.cvm_post_process(ctypes.byref(cout), float(post[0]), float(post[1]))
    return out


def coverage(in_lens, in_w, in_h, out_lens, out_w, out_h, num_samples, rotation=None, detail=False):
    """The count plane (out_h, out_w) uint8 of a num_samples call; detail: also the coordinates (out_h, out_w, n * n, 2) and the
    rotated ray z (out_h, out_w, n * n) of every sub-sample, in the loop's order."""
    n2 = int(num_samples) ** 2
    plane = np.full((out_h, out_w), 255, dtype=np.uint8)
    sxy = np.empty((out_h, out_w, n2, 2), dtype=np.float32) if detail else None
    vz = np.empty((out_h, out_w, n2), dtype=np.float32) if detail else None
    cin = oracle._image(in_lens, in_w, in_h, 1, None)
    cout = oracle._image(out_lens, out_w, out_h, 1, None)
    keep, rp = oracle._rot(rotation)
    rc = lib().cvm_coverage(ctypes.byref(cin), ctypes.byref(cout), int(num_samples), rp, plane.ctypes.data,
                            sxy.ctypes.data if detail else None, vz.ctypes.data if detail else None)
    if rc != 0:
        raise ValueError(f"cvm_coverage: {rc}")
    return (plane, sxy, vz) if detail else plane


def masked(image, plane):
    """`image` (H, W, C) with every channel of the count-0 pixels set to +0.0f: what mask_image leaves."""
    out = np.array(image, dtype=np.float32, copy=True)
    out[plane == 0] = np.float32(0.0)
    return out


def alpha(plane, num_samples):
    """(float)count * (1.0f / (float)(n * n)), binary32."""
    normalize = np.float32(1.0) / np.float32(int(num_samples) ** 2)
    return plane.astype(np.float32) * normalize
