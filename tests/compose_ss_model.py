"""ctypes binding of tests/native/compose_ss_model.c — the CPU model of supersampled compose (include/lrp.h "compose,
supersampled"): the definition written out per pixel on the lens functions, samplers and coverage test of the coverage model
(tests/native/coverage_model.c, included textually).  Test infrastructure; built by __graft_entry__.build()."""
import ctypes
import os

import numpy as np

import oracle_binding as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "_build", "libcompose_ss_model.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        I = oracle.OImage  # same layout as cvm_image
        L.csm_compose.restype = ctypes.c_int
        L.csm_compose.argtypes = [P(I), ctypes.c_int, ctypes.c_void_p, P(I), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p]
        _lib = L
    return _lib


def compose(in_lenses, srcs, out_lens, out_w, out_h, num_samples, interpolation, rotations=None, mode=0, post=None):
    """The model's image (out_h, out_w, C) float32, count plane and coverage plane (out_h, out_w) uint8.  srcs: one (H, W, C)
    float32 array per source; rotations: one 3 x 3 matrix per source, or None; post: (exposure, reinhard) or None."""
    n = len(srcs)
    srcs = [np.ascontiguousarray(s, dtype=np.float32) for s in srcs]
    C = srcs[0].shape[2]
    arr = (oracle.OImage * n)()
    for i, (lens, s) in enumerate(zip(in_lenses, srcs)):
        arr[i] = oracle._image(lens, s.shape[1], s.shape[0], s.shape[2], s)
    out = np.full((out_h, out_w, C), np.float32(-12345.0), dtype=np.float32)
    count = np.full((out_h, out_w), 255, dtype=np.uint8)
    coverage = np.full((out_h, out_w), 255, dtype=np.uint8)
    cout = oracle._image(out_lens, out_w, out_h, C, out)
    rot = None if rotations is None else np.ascontiguousarray(np.asarray(rotations, dtype=np.float32).reshape(n, 9))
    cpost = None if post is None else np.array(post, dtype=np.float32)
    rc = lib().csm_compose(arr, n, None if rot is None else rot.ctypes.data, ctypes.byref(cout), int(num_samples), int(interpolation),
                           int(mode), None if cpost is None else cpost.ctypes.data, count.ctypes.data, coverage.ctypes.data)
    if rc != 0:
        raise ValueError(f"csm_compose: {rc}")
    return out, count, coverage
