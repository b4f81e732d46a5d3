"""The multi-band kernels: tools/isa_kernels.py over the built objects reports `scratch 0` and
`vgpr spilled 0` for all of them, and the LDS bytes the design states: (C + 1) x 7600 for multiband_reduce_kernel<C> (the 67 x 19
window in rows of 68 floats plus the 32 x 19 horizontal pass, per plane), C x 1200 for multiband_lap_kernel<C> and
multiband_collapse_kernel<C> (the 18 x 6 window plus the 32 x 6 horizontal pass, per channel), none for
multiband_label_kernel<OutLens> — exactly C = 1 .. 4 and 5 target lenses.  Resource figures only; no instruction text is read.
Skipped when the objects are not built."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj")
KERNEL = re.compile(r"^_ZN3lrp\d+multiband_(reduce|lap|collapse|label)_kernelILi(\d+)EEEvNS_\d+Multiband(Reduce|Lap|Collapse|Label)ParamsE$")
LDS = {"reduce": lambda c: (c + 1) * 19 * (68 + 32) * 4, "lap": lambda c: c * 6 * (18 + 32) * 4, "collapse": lambda c: c * 6 * (18 + 32) * 4,
       "label": lambda lens: 0}


def test_multiband_kernels_have_no_scratch_and_the_stated_lds(tmp_path):
    units = sorted(glob.glob(os.path.join(OBJ, "lrp_multiband*.o")))
    if len(units) < 2:
        pytest.skip("the kernel objects are not built")
    for u in units:  # (the tool takes a directory: one with these units alone, not the whole build)
        os.symlink(u, tmp_path / os.path.basename(u))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_kernels.py"), "kernels", str(tmp_path)], check=True, capture_output=True,
                         text=True).stdout
    found, vgprs = set(), {}
    for line in out.splitlines():
        f = line.split()
        res = dict(zip(f[2::2], f[3::2]))  # sgpr N spilled N vgpr N spilled N lds N scratch N: the second `spilled` is the VGPRs'
        vgpr_spilled = f[f.index("vgpr") + 3]
        m = KERNEL.match(f[0])
        if not m:
            assert "multiband" not in f[0], f"a kernel of another signature: {f[0]}"
            continue
        kind, arg = m.group(1), int(m.group(2))
        assert m.group(3).lower() == kind, line
        assert res["scratch"] == "0" and vgpr_spilled == "0" and int(res["lds"]) == LDS[kind](arg), line
        assert (kind, arg) not in found, line
        found.add((kind, arg))
        vgprs.setdefault(kind, []).append(int(res["vgpr"]))
    print("VGPRs per kernel:", {k: (min(v), max(v)) for k, v in sorted(vgprs.items())})
    want = {(k, c) for k in ("reduce", "lap", "collapse") for c in (1, 2, 3, 4)} | {("label", lens) for lens in range(5)}
    assert found == want, sorted(found ^ want)
