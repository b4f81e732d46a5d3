"""The cases of the calibrated-camera compose tests (include/lrp.h "compose, calibrated cameras"), shared by tests/test_camera.py
(CPU: the model against float64, the conventions against the existing lenses, lrp_camera_limit, the error table, and the rule
that every scene discriminates) and tests/test_gpu_camera.py (the HIP launch against the model of tests/camera_model.py, byte
for byte).

A camera is the dict of tests/camera_model.py; limit None means "ask lrp_camera_limit" (resolve())."""
import math

import numpy as np

import cases
import coverage_cases as cc

BROWN, FISHEYE = 0, 1
INF = float("inf")

# Brown-Conrady coefficients (k1 k2 p1 p2 k3) of a wide-angle lens with visible barrel distortion: r * L(r * r) turns near r = 1.86
BROWN_WIDE = (-0.28, 0.09, 0.001, -0.0007, -0.012)
BROWN_MILD = (0.05, -0.01, -0.002, 0.001, 0.001)
# Kannala-Brandt coefficients (k1 .. k4); td(theta) increases up to pi
FISHEYE_K = (-0.02, 0.003, -0.0005, 0.00005)


def camera(model, size, fx, fy, cx, cy, k, limit=None):
    return dict(model=model, size=size, fx=fx, fy=fy, cx=cx, cy=cy, k=tuple(k), limit=limit)


def product(lrp, cam, data=None):
    """The package's Camera of a case camera (limit None: lrp_camera_limit)."""
    w, h = cam["size"]
    return lrp.Camera(cam["model"], w, h, data, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["k"], cam["limit"])


def resolve(lrp, cam):
    """The camera with its limit filled in by lrp_camera_limit where it is None."""
    return cam if cam["limit"] is not None else dict(cam, limit=product(lrp, cam).limit)


# ---- the rig: three overlapping cameras of mixed models, off-centre principal points, fx != fy, every kind of coefficient
RIG = [
    camera(BROWN, (64, 48), 52.0, 51.0, 31.2, 23.8, BROWN_WIDE),
    camera(FISHEYE, (56, 40), 44.0, 43.0, 27.1, 19.6, FISHEYE_K),
    camera(BROWN, (64, 48), 58.0, 59.0, 32.4, 22.9, BROWN_MILD),
]
RIG_ROTATIONS = [(-24.0, 4.0, 0.0), (22.0, 10.0, 0.0), (3.0, -20.0, 8.0)]  # pan, pitch, roll relative to the target's axis
OUT_SIZE = (80, 48)
OUT_LENSES = cc.OUT_LENSES  # the five target lenses, the extension bits on


def rig(lrp, out_name, size=OUT_SIZE):
    """(output lens, cameras, rotation matrices) of the rig in front of target lens out_name.  The fisheye targets look along
    +z, the others along -z: the rig is turned to face the target."""
    base = 180.0 if out_name in ("eqd_pi", "eqs", "stg") else 0.0
    rots = [cases.rotation(lrp, (base + pan, pitch, roll)) for pan, pitch, roll in RIG_ROTATIONS]
    return cc.lens(lrp, out_name, size[0], size[1]), [resolve(lrp, c) for c in RIG], rots


def sources(cams, channels=4, seed=700, planted=False):
    """The noise frames of the cameras; without planted texels none is zero (+0.25), so that a zero pixel is an uncovered one."""
    noise = [cases.hash_noise(c["size"][1], c["size"][0], channels, seed + i, planted=planted) for i, c in enumerate(cams)]
    if not planted:
        return [a + np.float32(0.25) for a in noise]
    # besides the six texels hash_noise plants somewhere: a 3 x 3 block of special values at the principal point, which the rig's
    # scenes look at
    special = np.array([-0.0, 1e-41, np.inf, np.nan, -np.inf, 3.0e38, 65504.0, -7.25, 1.0], dtype=np.float32)
    for a, c in zip(noise, cams):
        x0, y0 = int(round(c["cx"])) - 1, int(round(c["cy"])) - 1
        for j in range(9):
            a[y0 + j // 3, x0 + j % 3, :] = np.roll(special, j)[:channels] if channels <= 9 else special[j]
    return noise


def discriminates(count, m, n):
    """The four conditions every scene of the GPU test has to meet."""
    return bool((m == 0).any() and ((m > 0) & (m < n * n)).any() and (m == n * n).any() and (count >= 2).any())


# ---- a 200 degree fisheye (theta up to 1.75 rad) and a full panorama: it sees behind itself
FISHEYE_200 = camera(FISHEYE, (64, 64), 18.0, 18.0, 31.5, 31.5, (0.01, -0.002, 0.0, 0.0), limit=1.75)

# ---- identity: a rectilinear 64 x 32 target (focal 16 on a 32 x 16 sensor) and an undistorted camera of the same pinhole
IDENTITY = camera(BROWN, (64, 32), 32.0, 32.0, 31.5, 15.5, (0.0, 0.0, 0.0, 0.0, 0.0), limit=INF)


def identity_lens(lrp):
    return lrp.LensInfo(0, (16.0, 0.0, 0.0, 0.0), 32.0, 16.0)


def eight(lrp):
    """Eight cameras of alternating models round the horizon, and their rotations."""
    cams, rots = [], []
    for i in range(8):
        base = RIG[i % 2]
        cams.append(resolve(lrp, dict(base, size=(base["size"][0] - 8 * (i % 3 == 2), base["size"][1]))))
        rots.append(cases.rotation(lrp, (35.0 * i, 10.0 * (i % 3) - 10.0, 0.0)))
    return cams, rots


# ---- float64 restatement of the two mappings (tests/test_camera.py): written from the formulas, not from the C file
def project64(cam, rays):
    v = np.asarray(rays, dtype=np.float64)
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    k = list(cam["k"]) + [0.0] * (5 - len(cam["k"]))
    k = [float(np.float32(c)) for c in k]
    fx, fy, cx, cy = (float(np.float32(cam[n])) for n in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        if cam["model"] == FISHEYE:
            rho = np.hypot(vx, vy)
            theta = np.arctan2(rho, -vz)
            t2 = theta * theta
            td = theta * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
            q = np.where(rho > 0, td / np.where(rho > 0, rho, 1.0), 0.0)
            return np.stack([fx * q * vx + cx, fy * q * vy + cy], axis=1)
        a, b = vx / -vz, vy / -vz
        r2 = a * a + b * b
        L = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]))
        xd = a * L + 2 * k[2] * a * b + k[3] * (r2 + 2 * a * a)
        yd = b * L + k[2] * (r2 + 2 * b * b) + 2 * k[3] * a * b
        return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def ray_grid(half_angle, steps=41):
    """Unit rays on a grid of directions round -z, up to half_angle off axis in x and in y."""
    t = np.linspace(-half_angle, half_angle, steps)
    ax, ay = np.meshgrid(t, t)
    x, y, z = np.sin(ax) * np.cos(ay), np.sin(ay), -np.cos(ax) * np.cos(ay)
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


PI = math.pi
