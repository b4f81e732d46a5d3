"""ctypes binding of tests/native/camera_gain_model.c — the CPU model of exposure matching across a camera rig (include/lrp.h
"exposure matching across a camera rig"): the overlap statistic and compose with one gain per camera, written out per pixel
from the header on the lenses, samplers and camera polynomials of tests/native/camera_model.c (included textually).  Test
infrastructure; built by __graft_entry__.build().

A camera is the dict of tests/camera_model.py."""
import ctypes
import os

import numpy as np

import camera_model as cmodel
import oracle_binding as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "_build", "libcamera_gain_model.so")
WORDS = 128
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        L.camg_overlap.restype = ctypes.c_int
        L.camg_overlap.argtypes = [P(cmodel.CCamera), ctypes.c_int, ctypes.c_void_p, P(oracle.OImage), ctypes.c_float, ctypes.c_float,
                                   ctypes.c_void_p]
        L.camg_compose.restype = ctypes.c_int
        L.camg_compose.argtypes = [P(cmodel.CCamera), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, P(oracle.OImage), ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def _cameras(cams, srcs):
    srcs = [np.ascontiguousarray(s, dtype=np.float32) for s in srcs]
    C = srcs[0].shape[2]
    arr = (cmodel.CCamera * len(cams))()
    for i, (cam, s) in enumerate(zip(cams, srcs)):
        assert s.shape == (cam["size"][1], cam["size"][0], C)
        arr[i] = cmodel.c_camera(cam, s)
    return arr, srcs, C


def _rotations(rotations, n):
    return None if rotations is None else np.ascontiguousarray(np.asarray(rotations, dtype=np.float32).reshape(n, 9))


def overlap(cams, srcs, out_lens, out_w, out_h, rotations=None, lo=0.02, hi=0.98):
    """The model's table, int64 (8, 8, 2): [i, j] = (N_ij, S_ij)."""
    n = len(cams)
    arr, srcs, C = _cameras(cams, srcs)
    stats = np.full(WORDS, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # (the model writes every word)
    cout = oracle._image(out_lens, out_w, out_h, C, None)
    rot = _rotations(rotations, n)
    rc = lib().camg_overlap(arr, n, None if rot is None else rot.ctypes.data, ctypes.byref(cout), float(lo), float(hi), stats.ctypes.data)
    if rc != 0:
        raise ValueError(f"camg_overlap: {rc}")
    return stats.astype(np.int64).reshape(8, 8, 2)


def compose(cams, srcs, gains, out_lens, out_w, out_h, num_samples, interpolation, rotations=None, mode=0, post=None):
    """camera_model.compose() with one gain per camera: the image, the count plane and the coverage plane."""
    n = len(cams)
    arr, srcs, C = _cameras(cams, srcs)
    g = np.ascontiguousarray(np.asarray(gains, dtype=np.float32).reshape(n))
    out = np.full((out_h, out_w, C), np.float32(-12345.0), dtype=np.float32)
    count = np.full((out_h, out_w), 255, dtype=np.uint8)
    coverage = np.full((out_h, out_w), 255, dtype=np.uint8)
    cout = oracle._image(out_lens, out_w, out_h, C, out)
    rot = _rotations(rotations, n)
    cpost = None if post is None else np.array(post, dtype=np.float32)
    rc = lib().camg_compose(arr, n, None if rot is None else rot.ctypes.data, g.ctypes.data, ctypes.byref(cout), int(num_samples),
                            int(interpolation), int(mode), None if cpost is None else cpost.ctypes.data, count.ctypes.data,
                            coverage.ctypes.data)
    if rc != 0:
        raise ValueError(f"camg_compose: {rc}")
    return out, count, coverage
