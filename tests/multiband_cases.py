"""The cases of the multi-band blending tests (include/lrp.h "multi-band blending across a camera rig"), shared by
tests/test_multiband.py (CPU: the model of tests/multiband_model.py against the numpy restatement below, the winner rule,
reconstruction, the discrimination of blending, the error tables) and tests/test_gpu_multiband.py (the HIP launches against the
model, byte for byte).  The rig and its frames are tests/camera_cases.py's, the recovery scene tests/camera_gain_cases.py's."""
import numpy as np

import camera_cases as cam
import camera_gain_cases as gc
import cases

F32 = np.float32
NO_CAMERA = 255
BANDS = 3  # of the cell cases

# ---- measured with the CPU model (tests/test_multiband.py prints them; DESIGN.md section 22 records them)
# reconstruction: one camera covers the target; max |result - render| in ulps of the render's largest value, per B.  The bound
# is twice that.
RECONSTRUCTION_ULPS_MEASURED = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1}
# the recovery scene without gains: the largest |difference| between 4-neighbours that two different cameras win, colour channels
SEAM_STEP_MEASURED = {0: 0.35923, 4: 0.17502}
# the recovery scene with equal exposures: max |multiband(B = 4) - FEATHER| over the covered pixels, colour channels
# (large: at 80 x 48 the rig's overlaps are narrower than 2^4 pixels, so the low bands reach past a camera's coverage, where
# its image is zero)
FEATHER_DIFFERENCE_MEASURED = 0.17869


def levels(w, h, bands):
    out = [(w, h)]
    for _ in range(bands):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        out.append((w, h))
    return out


def round256(n):
    return (n + 255) & ~255


def scratch_bytes(w, h, channels, bands):
    """The layout include/lrp.h states: per level one camera's G_k and (above level 0) M_k, the accumulators A_k and S_k; then a
    label and a count plane; every region rounded up to 256 bytes."""
    total = 0
    for k, (wk, hk) in enumerate(levels(w, h, bands)):
        px = wk * hk
        total += round256(px * channels * 4) + (round256(px * 4) if k > 0 else 0) + round256(px * channels * 4) + round256(px * 4)
    return total + 2 * round256(w * h)


# ---- the numpy float32 restatement of reduce, expand, accumulate and collapse: elementwise float32 operations are un-fused
# and correctly rounded, so it is comparable bit for bit.  Arrays are (h, w, P).
def _ix(j, w, wrap):
    return np.mod(j, w) if wrap else np.clip(j, 0, w - 1)


def _tap5(p):
    return (((p[0] + p[4]) + F32(4.0) * (p[1] + p[3])) + F32(6.0) * p[2]) * F32(0.0625)


def reduce_np(a, wrap):
    h, w = a.shape[:2]
    x, y = np.arange((w + 1) >> 1), np.arange((h + 1) >> 1)
    hor = _tap5([a[:, _ix(2 * x + d, w, wrap)] for d in (-2, -1, 0, 1, 2)])
    out = _tap5([hor[np.clip(2 * y + d, 0, h - 1)] for d in (-2, -1, 0, 1, 2)])
    assert out.dtype == np.float32
    return out


def _expand_axis(c, n, axis, wrap):
    """c along `axis` (coarse) -> n entries."""
    c = np.moveaxis(c, axis, 0)
    cn = c.shape[0]
    j = np.arange(n)
    i = j >> 1
    cm, c0, c1 = c[_ix(i - 1, cn, wrap)], c[i], c[_ix(i + 1, cn, wrap)]
    even = ((cm + c1) + F32(6.0) * c0) * F32(0.125)
    odd = (c0 + c1) * F32(0.5)
    odd_mask = (j & 1).astype(bool).reshape((-1,) + (1,) * (c.ndim - 1))
    return np.moveaxis(np.where(odd_mask, odd, even), 0, axis)


def expand_np(c, w, h, wrap):
    out = _expand_axis(_expand_axis(c, w, 1, wrap), h, 0, False)
    assert out.dtype == np.float32
    return out


def blend_np(layers, label, bands, wrap, post=None):
    """The definition from the level-0 layers G^i_0 (h, w, C) and the label plane."""
    with np.errstate(all="ignore"):
        A, S = None, None
        for i, g0 in enumerate(layers):
            G, M = [g0.astype(np.float32)], [(label == i).astype(np.float32)[..., None]]
            for k in range(bands):
                G.append(reduce_np(G[k], wrap)), M.append(reduce_np(M[k], wrap))
            if A is None:
                A, S = [np.zeros_like(g) for g in G], [np.zeros_like(m) for m in M]
            for k in range(bands + 1):
                L = G[k] - expand_np(G[k + 1], G[k].shape[1], G[k].shape[0], wrap) if k < bands else G[k]
                A[k] = A[k] + np.where(M[k] == 0, F32(0.0), M[k] * L)
                S[k] = S[k] + M[k]
        R = None
        for k in range(bands, -1, -1):
            N = np.where(S[k] > 0, A[k] / np.where(S[k] > 0, S[k], F32(1.0)), F32(0.0))
            R = N if k == bands else N + expand_np(R, N.shape[1], N.shape[0], wrap)
        out = R.astype(np.float32)
        if post is not None:
            e, r = F32(post[0]), F32(post[1])
            t = out[..., :3] * e
            out[..., :3] = t * (F32(1.0) + t / (r * r)) / (F32(1.0) + t)
        out[label == NO_CAMERA] = F32(0.0)
    assert out.dtype == np.float32
    return out


def ulps_of_scale(a, b):
    """|a - b| in units of the last place of b's largest magnitude, float32."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / float(np.spacing(np.abs(b).max()))


def seam_step(img, label):
    """The largest |difference| of the colour channels between 4-neighbours that two different cameras win."""
    best = 0.0
    col = img[..., :3].astype(np.float64)
    for a, b, la, lb in ((col[:, 1:], col[:, :-1], label[:, 1:], label[:, :-1]), (col[1:], col[:-1], label[1:], label[:-1])):
        seam = (la != lb) & (la != NO_CAMERA) & (lb != NO_CAMERA)
        if seam.any():
            best = max(best, float(np.abs(a - b)[seam].max()))
    return best


# ---- scenes
def seam_rig(lrp, out_name, size=cam.OUT_SIZE):
    """The rig turned by 180 degrees, so that in an equirectangular target it straddles the +-180 degree seam."""
    import coverage_cases as cc

    rots = [cases.rotation(lrp, (180.0 + pan, pitch, roll)) for pan, pitch, roll in cam.RIG_ROTATIONS]
    return cc.lens(lrp, out_name, size[0], size[1]), [cam.resolve(lrp, c) for c in cam.RIG], rots


def cut_lens(lrp):
    """eqr_band cut to less than a full turn: clamps in x."""
    return lrp.LensInfo.equirectangular(-3.0, 3.0, -0.5, 0.5)


def equal_exposure_scene(lrp):
    lout, cams, rots, srcs = gc.recovery_scene(lrp)
    out = []
    for s, e in zip(srcs, gc.EXPOSURES):
        t = s.copy()
        t[..., :3] = s[..., :3] / F32(e)
        out.append(t)
    return lout, cams, rots, out
