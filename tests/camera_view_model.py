"""ctypes binding of tests/native/camera_view_model.c — the CPU model of compose into a calibrated target camera (include/lrp.h
"calibrated camera as the target"): the definition written out per pixel, on the source mapping, samplers and libm of the camera
model (tests/native/camera_model.c, included textually) with the Newton inverse written from the header.  Test infrastructure;
built by __graft_entry__.build().

A camera is the dict of tests/camera_model.py."""
import ctypes
import os

import numpy as np

from camera_model import CCamera, c_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "_build", "libcamera_view_model.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        L.camview_unproject.restype = ctypes.c_int
        L.camview_unproject.argtypes = [P(CCamera), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.camview_detail.restype = ctypes.c_int
        L.camview_detail.argtypes = [P(CCamera), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.camview_compose.restype = ctypes.c_int
        L.camview_compose.argtypes = [P(CCamera), ctypes.c_int, ctypes.c_void_p, P(CCamera), ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def unproject(cam, uv):
    """uv (N, 2) float32, pixels -> rays (N, 3) float32, has_ray (N,) bool."""
    uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
    n = uv.shape[0]
    rays = np.empty((n, 3), dtype=np.float32)
    has = np.empty(n, dtype=np.uint8)
    c = c_camera(cam)
    if lib().camview_unproject(ctypes.byref(c), uv.ctypes.data, n, rays.ctypes.data, has.ctypes.data) != 0:
        raise ValueError("camview_unproject")
    return rays, has.astype(bool)


def detail(target, num_samples):
    """Per sub-sample of the target, (H, W, n * n) in the loop's order: the position u, v (.., 2), the ray (.., 3), has_ray."""
    w, h = target["size"]
    n2 = num_samples * num_samples
    uv = np.empty((h, w, n2, 2), dtype=np.float32)
    ray = np.empty((h, w, n2, 3), dtype=np.float32)
    has = np.empty((h, w, n2), dtype=np.uint8)
    c = c_camera(target)
    if lib().camview_detail(ctypes.byref(c), int(num_samples), uv.ctypes.data, ray.ctypes.data, has.ctypes.data) != 0:
        raise ValueError("camview_detail")
    return uv, ray, has.astype(bool)


def compose(cams, srcs, target, num_samples, interpolation, rotations=None, mode=0, post=None):
    """The model's image (h, w, C) float32, count plane and coverage plane (h, w) uint8 of the target's frame.  srcs: one
    (H, W, C) float32 array per camera; rotations: one 3 x 3 matrix per camera, or None; post: (exposure, reinhard) or None."""
    n = len(cams)
    srcs = [np.ascontiguousarray(s, dtype=np.float32) for s in srcs]
    C = srcs[0].shape[2]
    arr = (CCamera * n)()
    for i, (cam, s) in enumerate(zip(cams, srcs)):
        assert s.shape == (cam["size"][1], cam["size"][0], C)
        arr[i] = c_camera(cam, s)
    w, h = target["size"]
    out = np.full((h, w, C), np.float32(-12345.0), dtype=np.float32)
    count = np.full((h, w), 255, dtype=np.uint8)
    coverage = np.full((h, w), 255, dtype=np.uint8)
    ct = c_camera(target)
    rot = None if rotations is None else np.ascontiguousarray(np.asarray(rotations, dtype=np.float32).reshape(n, 9))
    cpost = None if post is None else np.array(post, dtype=np.float32)
    rc = lib().camview_compose(arr, n, None if rot is None else rot.ctypes.data, ctypes.byref(ct), out.ctypes.data, C, int(num_samples),
                               int(interpolation), int(mode), None if cpost is None else cpost.ctypes.data, count.ctypes.data,
                               coverage.ctypes.data)
    if rc != 0:
        raise ValueError(f"camview_compose: {rc}")
    return out, count, coverage
