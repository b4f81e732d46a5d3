"""ctypes binding of tests/native/multiband_model.c — the CPU model of multi-band blending across a camera rig (include/lrp.h
"multi-band blending across a camera rig"): the labels, the level-0 layers, the pyramid, the accumulation and the collapse written
out from the header on the camera models of tests/native/camera_model.c and camera_gain_model.c (included textually).  Test
infrastructure; built by __graft_entry__.build().

A camera is the dict of tests/camera_model.py."""
import ctypes
import os

import numpy as np

import camera_gain_model as gmodel
import camera_model as cmodel
import oracle_binding as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "_build", "libmultiband_model.so")
NO_CAMERA = 255
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        L.mbm_labels.restype = ctypes.c_int
        L.mbm_labels.argtypes = [P(cmodel.CCamera), ctypes.c_int, ctypes.c_void_p, P(oracle.OImage), ctypes.c_void_p, ctypes.c_void_p]
        L.mbm_compose.restype = ctypes.c_int
        L.mbm_compose.argtypes = [P(cmodel.CCamera), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, P(oracle.OImage), ctypes.c_int, ctypes.c_int,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def labels(cams, out_lens, out_w, out_h, rotations=None):
    """(count, label) planes (out_h, out_w) uint8; no frame is read."""
    n = len(cams)
    arr = (cmodel.CCamera * n)(*[cmodel.c_camera(c) for c in cams])
    count = np.full((out_h, out_w), 254, dtype=np.uint8)
    label = np.full((out_h, out_w), 254, dtype=np.uint8)
    cout = oracle._image(out_lens, out_w, out_h, 1, None)
    rot = gmodel._rotations(rotations, n)
    rc = lib().mbm_labels(arr, n, None if rot is None else rot.ctypes.data, ctypes.byref(cout), count.ctypes.data, label.ctypes.data)
    if rc != 0:
        raise ValueError(f"mbm_labels: {rc}")
    return count, label


def compose(cams, srcs, out_lens, out_w, out_h, interpolation, rotations=None, num_bands=5, gains=None, post=None):
    """The model's image (out_h, out_w, C) float32, the count plane and the label plane (out_h, out_w) uint8."""
    n = len(cams)
    arr, srcs, C = gmodel._cameras(cams, srcs)
    g = None if gains is None else np.ascontiguousarray(np.asarray(gains, dtype=np.float32).reshape(n))
    out = np.full((out_h, out_w, C), np.float32(-12345.0), dtype=np.float32)
    count = np.full((out_h, out_w), 254, dtype=np.uint8)
    label = np.full((out_h, out_w), 254, dtype=np.uint8)
    cout = oracle._image(out_lens, out_w, out_h, C, out)
    rot = gmodel._rotations(rotations, n)
    cpost = None if post is None else np.array(post, dtype=np.float32)
    rc = lib().mbm_compose(arr, n, None if rot is None else rot.ctypes.data, None if g is None else g.ctypes.data, ctypes.byref(cout),
                           int(interpolation), int(num_bands), None if cpost is None else cpost.ctypes.data, count.ctypes.data, label.ctypes.data)
    if rc != 0:
        raise ValueError(f"mbm_compose: {rc}")
    return out, count, label
