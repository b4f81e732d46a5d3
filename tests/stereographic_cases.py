"""Whole frames of the stereographic lens extension: the little planet (a full 4096 x 2048 equirectangular panorama rendered
whole into one 2048^2 stereographic frame, looking at the pole) and the BASELINE configs[1] twin with the stereographic lens in
place of the equidistant stand-in.  Shared by tests/golden/make_stereographic_golden.py (renders them with the CPU model,
tests/stereographic_model.py, and commits the digests) and tests/test_gpu_stereographic_golden.py (the HIP path against the
committed digests).  Source = the counter-based synthetic frame (seed, depth channel); digests as tests/fullframe_cases.py
frame_digests."""

NEAREST, BILINEAR, BICUBIC = 0, 1, 2


def lens(lrp, name, w, h):
    if name == "stg":  # 12.5 mm behind a 36 mm sensor: the image circle of theta = 90 degrees touches r = 25 mm
        return lrp.LensInfo.stereographic(12.5, 36.0, w, h)
    if name == "stg_planet":  # 2 mm: the frame's edge (r = 18 mm, t = 4.5) is at theta = 155 degrees, its corner at 162
        return lrp.LensInfo.stereographic(2.0, 36.0, w, h)
    if name == "rect":
        return lrp.LensInfo.rectilinear(18.0, 36.0, w, h)
    if name == "eqr_full":
        return lrp.LensInfo.equirectangular()
    raise KeyError(name)


def _case(name, c, inp, out, interp, deg, seed, in_size, out_size, depth=-1, post=None):
    return dict(name=name, in_size=list(in_size), out_size=list(out_size), c=c, inp=inp, out=out, interp=interp, deg=deg, seed=seed,
                depth=depth, post=post)


def frame_cases():
    cs = [
        _case("stg_little_planet_eqr_stg_bc", 4, "eqr_full", "stg_planet", BICUBIC, (0.0, 90.0, 0.0), 0x5EED0000, (4096, 2048), (2048, 2048)),
        _case("stg_config1_4k_stg_rect_bc", 4, "stg", "rect", BICUBIC, None, 0x5EED0000, (4096, 4096), (4096, 4096)),
    ]
    return {c["name"]: c for c in cs}
