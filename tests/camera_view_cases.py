"""The cases of the camera-view tests (include/lrp.h "calibrated camera as the target"), shared by tests/test_camera_view.py (CPU:
lrp_camera_unproject against the model bit for bit, the model against float64, the pinhole target against the rectilinear
lens, +inf and NaN, the error table, and the rule that every scene discriminates) and tests/test_gpu_camera_view.py (the HIP
launch against the model of tests/camera_view_model.py, byte for byte).

Cameras are the dicts of tests/camera_cases.py; the sources are its RIG with RIG_ROTATIONS, in front of a target that looks
down -z."""
import numpy as np

import camera_cases as cam
import cases

BROWN, FISHEYE, INF = cam.BROWN, cam.FISHEYE, cam.INF

# ---- the target cameras.  limit None: lrp_camera_limit (resolve()).
TARGETS = {
    # the wide lens in a frame larger than its field: r * L(r * r) turns near r = 1.86, where it is 1.137 — 18.2 px from the
    # principal point at fx = 16 —, so the 40 % of the 48 x 36 frame outside that disc has no ray
    "brown_clipped": cam.camera(BROWN, (48, 36), 16.0, 16.0, 23.3, 17.6, cam.BROWN_WIDE),
    # the same lens with the rig's own focal lengths: every pixel has a ray
    "brown_wide": cam.camera(BROWN, (64, 48), 52.0, 51.0, 31.2, 23.8, cam.BROWN_WIDE),
    # fx != fy and the principal point well off the centre
    "brown_mild": cam.camera(BROWN, (64, 48), 24.0, 27.0, 25.6, 28.9, cam.BROWN_MILD),
    "fisheye": cam.camera(FISHEYE, (56, 40), 24.0, 23.0, 27.1, 19.6, cam.FISHEYE_K),
    # a fisheye whose limit lies inside the frame: theta = 1.2 is 21.6 px from the centre of a 64 x 64 frame
    "fisheye_clipped": dict(cam.FISHEYE_200, limit=1.2),
    # a pinhole (k = 0) whose principal point is off centre by a quarter of the frame: a new camera matrix
    "pinhole": cam.camera(BROWN, (64, 48), 30.0, 30.0, 31.5 + 16.0, 23.5 - 12.0, (0.0,) * 5, limit=INF),
}
CLIPPED = ("brown_clipped", "fisheye_clipped")  # targets with sub-samples that have no ray


def target(lrp, name):
    return cam.resolve(lrp, TARGETS[name])


def small_target(lrp, name, size):
    """The target `name` in a frame of another size, the principal point near the middle of it; fx = fy = 12, so that the ends of
    a 33 x 9 frame of the wide lens (r_d = 1.37 > 1.137) still have no ray."""
    return dict(target(lrp, name), size=size, fx=12.0, fy=12.0, cx=size[0] / 2 - 0.3, cy=size[1] / 2 - 0.7)


def rig(lrp):
    """(cameras, rotation matrices) of the rig of tests/camera_cases.py in front of a target that looks down -z."""
    return [cam.resolve(lrp, c) for c in cam.RIG], [cases.rotation(lrp, r) for r in cam.RIG_ROTATIONS]


def sub_positions(size, n):
    """u, v of every sub-sample, (H, W, n * n, 2) float32 in the loop's order (sub = n * ssx + ssy), by the definition's arithmetic."""
    w, h = size
    f = np.float32
    off = (np.arange(n, dtype=f) + f(1.0)) / (f(n) + f(1.0))
    u = (np.arange(w, dtype=f)[:, None] + off[None, :]) - f(0.5)  # (W, n)
    v = (np.arange(h, dtype=f)[:, None] + off[None, :]) - f(0.5)  # (H, n)
    out = np.empty((h, w, n, n, 2), dtype=f)
    out[..., 0] = u[None, :, :, None]
    out[..., 1] = v[:, None, None, :]
    return out.reshape(h, w, n * n, 2)


# ---- float64: Newton to convergence with the definition's sticky rule, written from the formulas, not from the C file
def unproject64(c, uv, steps=80):
    """uv (N, 2) -> rays (N, 3) float64, has_ray (N,), and the quantity `limit` bounds at the solution (r2 / theta)."""
    uv = np.asarray(uv, dtype=np.float64)
    k = [float(np.float32(x)) for x in list(c["k"]) + [0.0] * (5 - len(c["k"]))]
    fx, fy, cx, cy, limit = (float(np.float32(c[name])) for name in ("fx", "fy", "cx", "cy", "limit"))
    x0, y0 = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
    with np.errstate(all="ignore"):
        if c["model"] == FISHEYE:
            rd = np.hypot(x0, y0)
            g = lambda t: t * (1 + t * t * (k[0] + t * t * (k[1] + t * t * (k[2] + t * t * k[3]))))
            th = rd.copy()
            ok = th <= limit
            for _ in range(steps):
                t2 = th * th
                gp = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
                th = th - (g(th) - rd) / gp
                ok &= (th >= 0) & (th <= limit)
            e = g(th) - rd
            has = ok & (np.abs(fx * e) <= 0.5) & (np.abs(fy * e) <= 0.5)
            q = np.where(rd > 0, np.sin(th) / np.where(rd > 0, rd, 1.0), 0.0)
            return np.stack([q * x0, q * y0, -np.cos(th)], axis=1), has, th
        k1, k2, p1, p2, k3 = k

        def forward(X, Y):
            r2 = X * X + Y * Y
            L = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            return X * L + 2 * p1 * X * Y + p2 * (r2 + 2 * X * X), Y * L + p1 * (r2 + 2 * Y * Y) + 2 * p2 * X * Y, r2, L

        X, Y = x0.copy(), y0.copy()
        ok = X * X + Y * Y <= limit
        for _ in range(steps):
            xd, yd, r2, L = forward(X, Y)
            D = k1 + r2 * (2 * k2 + r2 * 3 * k3)
            ex, ey = xd - x0, yd - y0
            jxx = L + 2 * X * X * D + 2 * p1 * Y + 6 * p2 * X
            jxy = 2 * X * Y * D + 2 * p1 * X + 2 * p2 * Y
            jyy = L + 2 * Y * Y * D + 6 * p1 * Y + 2 * p2 * X
            det = jxx * jyy - jxy * jxy
            X, Y = X - (jyy * ex - jxy * ey) / det, Y - (jxx * ey - jxy * ex) / det
            ok &= X * X + Y * Y <= limit
        xd, yd, r2, _ = forward(X, Y)
        has = ok & (np.abs(fx * (xd - x0)) <= 0.5) & (np.abs(fy * (yd - y0)) <= 0.5)
        return np.stack([X, Y, -np.ones_like(X)], axis=1), has, r2
