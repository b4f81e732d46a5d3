"""The frame-loop window kernels that read the geometry cache own no scratch memory: tools/isa_kernels.py over the built
objects reports `scratch 0` and `vgpr spilled 0` for every reproject_bicubic_win_kernel<..., Frames, GeoRead, !SS>, at no more
than 128 vector registers where four wavefronts per SIMD are asked for (RGB / RGBA).  Skipped when the objects are not built."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj")
# reproject_bicubic_win_kernel<OutLens, InMode, QMode, CH, Frames = true, GeoRead = true, SS = false>, Itanium-mangled
FRAME_GEO = re.compile(r"^_ZN3lrp28reproject_bicubic_win_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb1ELb1ELb0EEEvNS_7KParamsE$")


def test_frame_loop_geo_kernels_have_no_scratch():
    units = [f"lrp_tile_wing{s}.o" for s in ("", "3", "5")]
    if not all(os.path.exists(os.path.join(OBJ, u)) for u in units):
        pytest.skip("the kernel objects are not built")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_kernels.py"), "kernels", OBJ], check=True, capture_output=True,
                         text=True).stdout
    seen = set()
    for line in out.splitlines():
        f = line.split()
        m = FRAME_GEO.match(f[0])
        if not m:
            continue
        res = dict(zip(f[2::2], f[3::2]))  # sgpr N spilled N vgpr N spilled N lds N scratch N: the second `spilled` is the VGPRs'
        vgpr_spilled = f[f.index("vgpr") + 3]
        in_mode, ch = int(m.group(2)), int(m.group(4))
        seen.add((in_mode, ch))
        assert res["scratch"] == "0" and vgpr_spilled == "0", line
        if ch != 5:  # (RGBAZ: three wavefronts per SIMD)
            assert int(res["vgpr"]) <= 128, line
    assert seen == {(m, c) for m in range(4) for c in (3, 4, 5)}, sorted(seen)
