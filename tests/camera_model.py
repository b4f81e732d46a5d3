"""ctypes binding of tests/native/camera_model.c — the CPU model of compose with calibrated cameras (include/lrp.h "compose,
calibrated cameras"): the definition written out per pixel, with the target lenses, samplers and libm of the coverage model
(tests/native/coverage_model.c, included textually) and the two camera polynomials written from the header.  Test
infrastructure; built by __graft_entry__.build().

A camera is a dict: model (0 BROWN, 1 FISHEYE), size (w, h), fx, fy, cx, cy, k (up to 5 floats), limit."""
import ctypes
import os

import numpy as np

import oracle_binding as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "_build", "libcamera_model.so")
BROWN, FISHEYE = 0, 1
_lib = None


class CCamera(ctypes.Structure):  # cam_camera == lrp_camera
    _fields_ = [("model", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("data", ctypes.c_void_p),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("k", ctypes.c_float * 5), ("limit", ctypes.c_float)]


assert ctypes.sizeof(CCamera) == 64


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        L.cam_project_rays.restype = None
        L.cam_project_rays.argtypes = [P(CCamera), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.cam_detail.restype = ctypes.c_int
        L.cam_detail.argtypes = [P(CCamera), P(oracle.OImage), ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.cam_compose.restype = ctypes.c_int
        L.cam_compose.argtypes = [P(CCamera), ctypes.c_int, ctypes.c_void_p, P(oracle.OImage), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def c_camera(cam, data=None):
    c = CCamera()
    c.model = int(cam["model"])
    c.width, c.height = cam["size"]
    c.data = None if data is None else data.ctypes.data
    c.fx, c.fy, c.cx, c.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    k = list(cam.get("k", ())) + [0.0] * (5 - len(cam.get("k", ())))
    for i in range(5):
        c.k[i] = k[i]
    c.limit = cam["limit"]
    return c


def project(cam, rays):
    """rays (N, 3) float32 -> sxy (N, 2) float32, imaged (N,) bool."""
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    n = rays.shape[0]
    sxy = np.empty((n, 2), dtype=np.float32)
    imaged = np.empty(n, dtype=np.uint8)
    c = c_camera(cam)
    lib().cam_project_rays(ctypes.byref(c), rays.ctypes.data, n, sxy.ctypes.data, imaged.ctypes.data)
    return sxy, imaged.astype(bool)


def detail(cam, out_lens, out_w, out_h, num_samples, rotation=None):
    """Per sub-sample of one camera, (H, W, n * n) in the loop's order: the rotated ray (.., 3), sx, sy (.., 2), imaged and covered."""
    n2 = num_samples * num_samples
    ray = np.empty((out_h, out_w, n2, 3), dtype=np.float32)
    sxy = np.empty((out_h, out_w, n2, 2), dtype=np.float32)
    flags = np.empty((out_h, out_w, n2), dtype=np.uint8)
    c = c_camera(cam)
    cout = oracle._image(out_lens, out_w, out_h, 1, None)
    rot = None if rotation is None else np.ascontiguousarray(np.asarray(rotation, dtype=np.float32).reshape(9))
    rc = lib().cam_detail(ctypes.byref(c), ctypes.byref(cout), int(num_samples), None if rot is None else rot.ctypes.data, ray.ctypes.data,
                          sxy.ctypes.data, flags.ctypes.data)
    if rc != 0:
        raise ValueError(f"cam_detail: {rc}")
    return ray, sxy, (flags & 1).astype(bool), (flags & 2).astype(bool)


def compose(cams, srcs, out_lens, out_w, out_h, num_samples, interpolation, rotations=None, mode=0, post=None):
    """The model's image (out_h, out_w, C) float32, count plane and coverage plane (out_h, out_w) uint8.  srcs: one (H, W, C)
    float32 array per camera; rotations: one 3 x 3 matrix per camera, or None; post: (exposure, reinhard) or None."""
    n = len(cams)
    srcs = [np.ascontiguousarray(s, dtype=np.float32) for s in srcs]
    C = srcs[0].shape[2]
    arr = (CCamera * n)()
    for i, (cam, s) in enumerate(zip(cams, srcs)):
        assert s.shape == (cam["size"][1], cam["size"][0], C)
        arr[i] = c_camera(cam, s)
    out = np.full((out_h, out_w, C), np.float32(-12345.0), dtype=np.float32)
    count = np.full((out_h, out_w), 255, dtype=np.uint8)
    coverage = np.full((out_h, out_w), 255, dtype=np.uint8)
    cout = oracle._image(out_lens, out_w, out_h, C, out)
    rot = None if rotations is None else np.ascontiguousarray(np.asarray(rotations, dtype=np.float32).reshape(n, 9))
    cpost = None if post is None else np.array(post, dtype=np.float32)
    rc = lib().cam_compose(arr, n, None if rot is None else rot.ctypes.data, ctypes.byref(cout), int(num_samples), int(interpolation),
                           int(mode), None if cpost is None else cpost.ctypes.data, count.ctypes.data, coverage.ctypes.data)
    if rc != 0:
        raise ValueError(f"cam_compose: {rc}")
    return out, count, coverage
