"""The cases of the exposure-matching tests (include/lrp.h "exposure matching across a camera rig"), shared by
tests/test_camera_gain.py (CPU: the model against the definition, lrp_camera_gains against numpy, recovery, the error tables, and
the rule that every scene discriminates) and tests/test_gpu_camera_gain.py (the HIP launches against the model of
tests/camera_gain_model.py, the table as integers and the images byte for byte).  The rig and its frames are
tests/camera_cases.py's."""
import numpy as np

import camera_cases as cam
import coverage_cases as cc

# lo, hi per scene: the frames are noise in 0.25 .. 1.25, so this range excludes a good part of what two cameras both cover
RANGE = {"rect18": (0.6, 0.9), "eqd_pi": (0.6, 0.9), "eqs": (0.6, 0.9), "stg": (0.6, 0.9), "eqr_part": (0.6, 0.9), "eight": (0.6, 0.9)}
# pairs 01, 02, 12: (pixels both cover, pixels both valid) under RANGE, from the camera model
MEASURED = {"rect18": [(674, 375), (447, 258), (527, 326)], "eqr_part": [(711, 410), (514, 308), (553, 347)]}
GAINS = (0.7, 1.0, 1.6)  # of the gained-compose cases


def eight_scene(lrp):
    """Eight cameras round the horizon in a full panorama: neighbours overlap, opposite cameras do not."""
    cams, rots = cam.eight(lrp)
    return cc.lens(lrp, "eqr_full", 80, 48), cams, rots, cam.sources(cams)


def special_frame():
    """A 32 x 64 frame of one channel for the identity scene of tests/camera_cases.py (every texel is its own pixel): column x
    holds special[x // 6].  Returns the frame and the q of the five values that are valid under lo = 0, hi = 32768."""
    special = np.array([[1.0, -0.0, 1e-41, 0.5, 32768.0, -7.25, np.inf, np.nan, -np.inf, 3.0e38, 65504.0]], dtype=np.float32)
    frame = np.repeat(np.repeat(special, 32, axis=0), 6, axis=1)[:, :64, None].copy()
    return frame, [65536, 0, 0, 32768, 1 << 31]


# ---- recovery: three frames cut from one smooth world, a function of the ray direction, under known exposures
EXPOSURES = (0.7, 1.0, 1.4)
# max(g_i e_i) / min(g_i e_i) - 1 of the gains the model's statistic yields, measured with the CPU model (tests/test_camera_gain.py
# prints it), per (sigma_n, sigma_g); the test's bound is twice that.  Without gains the spread is 1.0.  With the default prior
# (sigma_g = 0.1) the gains stop well short of equalising — the prior pulls them to 1 —; with a weak prior (sigma_g = 10) what is
# left is the resampling error.
RECOVERY_SPREAD_MEASURED = {(10 / 255, 0.1): 0.28844, (10 / 255, 10.0): 6.9e-5}


def world(rays):
    """The world's colour (N, 3) float32 in the direction of the target's rays (N, 3): smooth and within 0.2 .. 0.8."""
    d = rays.astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    base = 0.5 + 0.18 * np.sin(2.0 * x + 0.3) * np.cos(1.5 * y) + 0.08 * z
    return np.stack([base + 0.04 * np.sin(3.0 * y), base, base - 0.04 * np.cos(2.5 * x)], axis=1).astype(np.float32)


def recovery_scene(lrp, out_name="eqr_part"):
    """(output lens, cameras, rotations, frames): frame i shows world() through camera i, times EXPOSURES[i]; alpha is 1."""
    lout, cams, rots = cam.rig(lrp, out_name)
    srcs = []
    for c, rot, e in zip(cams, rots, EXPOSURES):
        w, h = c["size"]
        ys, xs = np.mgrid[0:h, 0:w]
        uv = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)
        rays, has_ray = lrp.camera_unproject(cam.product(lrp, c), uv)
        # compose turns the target's ray r into the camera's v = R r, so r = R^T v
        R = np.asarray(rot, dtype=np.float64).reshape(3, 3)
        target_rays = np.where(has_ray[:, None], rays.astype(np.float64), np.array([0.0, 0.0, -1.0])) @ R
        frame = np.ones((h * w, 4), dtype=np.float32)
        frame[:, :3] = world(target_rays) * np.float32(e)
        srcs.append(frame.reshape(h, w, 4))
    return lout, cams, rots, srcs
