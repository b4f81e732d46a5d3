"""ctypes binding of tests/native/stereographic_model.c — the CPU model of the reprojection loop with all five lens types, the
stereographic lens extension (include/lrp.h LRP_LENS_EXT_STEREOGRAPHIC) included.  Test infrastructure; built by
__graft_entry__.build()."""
import ctypes
import os

import numpy as np

import oracle_binding as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "_build", "libstereographic_model.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.POINTER
        I = oracle.OImage  # same layout as stm_image
        L.stm_reproject.restype = ctypes.c_int
        L.stm_reproject.argtypes = [P(I), P(I), ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.stm_reproject_rows.restype = ctypes.c_int
        L.stm_reproject_rows.argtypes = [P(I), P(I), ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.stm_post_process.restype = None
        L.stm_post_process.argtypes = [P(I), ctypes.c_float, ctypes.c_float]
        L.stm_source_position.restype = None
        L.stm_source_position.argtypes = [P(I), P(I), ctypes.c_void_p, ctypes.c_float, ctypes.c_float, P(ctypes.c_float),
                                          P(ctypes.c_float)]
        L.stm_stereographic_to_vec.restype = None
        L.stm_stereographic_to_vec.argtypes = [P(oracle.OLens), ctypes.c_float, ctypes.c_float, ctypes.c_float, P(ctypes.c_float)]
        L.stm_vec_to_stereographic.restype = None
        L.stm_vec_to_stereographic.argtypes = [P(oracle.OLens), ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                           P(ctypes.c_float), P(ctypes.c_float)]
        _lib = L
    return _lib


def reproject(in_lens, src, out_lens, out_w, out_h, num_samples, interpolation, rotation=None, post=None, threads=1):
    """Model reproject(): src (H, W, C) float32 -> (out_h, out_w, C); post = (exposure, reinhard) applies post_process.
    threads > 1 renders row bands in parallel (rows are independent)."""
    L = lib()
    src = np.ascontiguousarray(src, dtype=np.float32)
    h, w, c = src.shape
    out = np.full((out_h, out_w, c), np.float32(-12345.0), dtype=np.float32)
    cin = oracle._image(in_lens, w, h, c, src)
    cout = oracle._image(out_lens, out_w, out_h, c, out)
    keep, rp = oracle._rot(rotation)
    if threads <= 1:
        rcs = [L.stm_reproject(ctypes.byref(cin), ctypes.byref(cout), int(num_samples), int(interpolation), rp)]
    else:
        from concurrent.futures import ThreadPoolExecutor

        bands = [(out_h * i // threads, out_h * (i + 1) // threads) for i in range(threads)]
        with ThreadPoolExecutor(threads) as ex:
            rcs = list(ex.map(lambda b: L.stm_reproject_rows(ctypes.byref(cin), ctypes.byref(cout), int(num_samples),
                                                             int(interpolation), rp, b[0], b[1]), bands))
    if any(rc != 0 for rc in rcs):
        raise ValueError(f"stm_reproject: {rcs}")
    if post is not None:
        L.stm_post_process(ctypes.byref(cout), float(post[0]), float(post[1]))
    return out


def stereographic_to_vec(lens, img_w, cx, cy):
    v = (ctypes.c_float * 3)()
    ol = oracle._lens(lens)
    lib().stm_stereographic_to_vec(ctypes.byref(ol), img_w, cx, cy, v)
    return np.array(list(v), dtype=np.float32)


def vec_to_stereographic(lens, img_w, x, y, z):
    cx, cy = ctypes.c_float(), ctypes.c_float()
    ol = oracle._lens(lens)
    lib().stm_vec_to_stereographic(ctypes.byref(ol), img_w, x, y, z, ctypes.byref(cx), ctypes.byref(cy))
    return np.float32(cx.value), np.float32(cy.value)
