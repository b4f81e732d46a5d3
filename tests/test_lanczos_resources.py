"""The Lanczos-3 kernels own no scratch memory: tools/isa_kernels.py over the built objects reports `scratch 0` and
`vgpr spilled 0` for every lanczos_kernel<OutLens, InMode, CH> (30 cells x {RGBA, run-time channels}) and every
lanczos_geo_kernel<Loop, CH>, and none of them uses LDS.  Skipped when the objects are not built."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj")
COMPUTE = re.compile(r"^_ZN3lrp14lanczos_kernelILi(\d+)ELi(\d+)ELi(\d+)EEEvNS_7KParamsE$")
GEO = re.compile(r"^_ZN3lrp18lanczos_geo_kernelILb([01])ELi(\d+)EEEvNS_7KParamsE$")


def test_lanczos_kernels_have_no_scratch(tmp_path):
    units = ["lrp_lanczos.o", "lrp_lanczos_geo.o"]
    if not all(os.path.exists(os.path.join(OBJ, u)) for u in units):
        pytest.skip("the kernel objects are not built")
    for u in units:  # (the tool takes a directory: one with the two units alone, not the whole build)
        os.symlink(os.path.join(OBJ, u), tmp_path / u)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_kernels.py"), "kernels", str(tmp_path)], check=True, capture_output=True,
                         text=True).stdout
    cells, geo = set(), set()
    for line in out.splitlines():
        f = line.split()
        mc, mg = COMPUTE.match(f[0]), GEO.match(f[0])
        if not mc and not mg:
            continue
        res = dict(zip(f[2::2], f[3::2]))  # sgpr N spilled N vgpr N spilled N lds N scratch N: the second `spilled` is the VGPRs'
        vgpr_spilled = f[f.index("vgpr") + 3]
        assert res["scratch"] == "0" and vgpr_spilled == "0" and res["lds"] == "0", line
        if mc:
            cells.add(tuple(int(g) for g in mc.groups()))
        else:
            geo.add((int(mg.group(1)), int(mg.group(2))))
    assert cells == {(o, m, c) for o in range(5) for m in range(6) for c in (0, 4)}, sorted(cells)
    assert geo == {(loop, c) for loop in (0, 1) for c in (0, 4)}, sorted(geo)
