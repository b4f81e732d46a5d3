"""The packed level-0 collapse of multi-band blending: tools/isa_kernels.py over the built object of
csrc/lrp_mb_packed.hip reports exactly four kernels, mb_collapse_packed_kernel<C> for C = 1 .. 4, each with `scratch 0`,
`vgpr spilled 0` and the LDS bytes the design states: C x 1200 (the 18 x 6 window plus the 32 x 6 horizontal pass, per channel)
+ 1024 (the 8-bit threshold table).  Resource figures only; no instruction text is read.  Skipped when the objects are not built."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj", "lrp_mb_packed.o")
KERNEL = re.compile(r"^_ZN3lrp\d+mb_collapse_packed_kernelILi(\d+)EEEvNS_\d+MbCollapsePackedParamsE$")


def test_packed_collapse_kernels_have_no_scratch_and_the_stated_lds(tmp_path):
    if not os.path.exists(UNIT):
        pytest.skip("the kernel objects are not built")
    os.symlink(UNIT, tmp_path / os.path.basename(UNIT))  # (the tool takes a directory: one with this unit alone, not the whole build)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_kernels.py"), "kernels", str(tmp_path)], check=True, capture_output=True,
                         text=True).stdout
    found, vgprs = set(), {}
    for line in out.splitlines():
        f = line.split()
        res = dict(zip(f[2::2], f[3::2]))  # sgpr N spilled N vgpr N spilled N lds N scratch N: the second `spilled` is the VGPRs'
        vgpr_spilled = f[f.index("vgpr") + 3]
        m = KERNEL.match(f[0])
        assert m, f"a kernel of another signature: {f[0]}"
        c = int(m.group(1))
        assert res["scratch"] == "0" and vgpr_spilled == "0" and int(res["lds"]) == c * 6 * (18 + 32) * 4 + 1024, line
        assert c not in found, line
        found.add(c)
        vgprs[c] = int(res["vgpr"])
    print("VGPRs per kernel:", vgprs)
    assert found == {1, 2, 3, 4}, sorted(found)
