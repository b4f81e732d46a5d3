"""Whole 4096^2 frames of the equisolid lens extension: the BASELINE configs[1] / configs[2] twins with the equisolid lens in
place of the equidistant stand-in, and RGBAZ + tonemap out of an equisolid frame into a panorama.  Shared by
tests/golden/make_equisolid_golden.py (renders them with the CPU model, tests/equisolid_model.py, and commits the digests)
and tests/test_gpu_equisolid_golden.py (the HIP path against the committed digests).  Source = the counter-based synthetic
frame (seed, depth channel); digests as tests/fullframe_cases.py frame_digests."""
import math

NEAREST, BILINEAR, BICUBIC = 0, 1, 2


def lens(lrp, name, w, h):
    if name == "eqs":  # the README's example lens: 12.5 mm behind a 36 mm sensor, a 180-degree image circle
        return lrp.LensInfo.equisolid(12.5, 36.0, math.pi, w, h)
    if name == "rect":
        return lrp.LensInfo.rectilinear(18.0, 36.0, w, h)
    if name == "eqr_full":
        return lrp.LensInfo.equirectangular()
    raise KeyError(name)


def _case(name, c, inp, out, interp, deg, seed, depth=-1, post=None, size=4096):
    return dict(name=name, size=size, out_size=size, c=c, inp=inp, out=out, interp=interp, deg=deg, seed=seed, depth=depth,
                post=post)


def frame_cases():
    cs = [
        _case("eqs_config1_4k_eqs_rect_bc", 4, "eqs", "rect", BICUBIC, None, 0x5EED0000),
        _case("eqs_config2_4k_eqr_eqs_bl_rot", 4, "eqr_full", "eqs", BILINEAR, (30.0, -15.0, 5.0), 0x5EED0000),
        _case("eqs_4k_rgbaz_eqs_eqr_bc_post", 5, "eqs", "eqr_full", BICUBIC, (0.0, 0.0, 0.0), 0x5EED0007, depth=4, post=(2.0, 4.0)),
    ]
    return {c["name"]: c for c in cs}
