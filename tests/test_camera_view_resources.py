"""The camera-view kernels own no scratch memory and no LDS: tools/isa_kernels.py over the built objects reports `scratch 0`,
`vgpr spilled 0` and `lds 0` for every camera_view_kernel<TargetModel, Interp>, and the instantiations are exactly 2 target
models x 3 samplers (the sources' models are a run-time branch).  Resource figures only; no instruction text is read.  Skipped
when the objects are not built."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj")
KERNEL = re.compile(r"^_ZN3lrp\d+camera_view_kernelILi(\d+)ELi(\d+)EEEvNS_\d+CameraViewParamsE$")


def test_camera_view_kernels_have_no_scratch_and_no_lds(tmp_path):
    units = sorted(glob.glob(os.path.join(OBJ, "lrp_camview*.o")))
    if len(units) < 3:
        pytest.skip("the kernel objects are not built")
    for u in units:  # (the tool takes a directory: one with these units alone, not the whole build)
        os.symlink(u, tmp_path / os.path.basename(u))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_kernels.py"), "kernels", str(tmp_path)], check=True, capture_output=True,
                         text=True).stdout
    found, vgprs = set(), {}
    for line in out.splitlines():
        f = line.split()
        m = KERNEL.match(f[0])
        if not m:
            assert "camera_view_kernel" not in f[0], f"a kernel of another signature: {f[0]}"
            continue
        res = dict(zip(f[2::2], f[3::2]))  # sgpr N spilled N vgpr N spilled N lds N scratch N: the second `spilled` is the VGPRs'
        vgpr_spilled = f[f.index("vgpr") + 3]
        assert res["scratch"] == "0" and vgpr_spilled == "0" and res["lds"] == "0", line
        key = tuple(int(g) for g in m.groups())
        assert key not in found, line
        found.add(key)
        vgprs[key] = int(res["vgpr"])
    print(f"{len(found)} kernels; VGPRs (target model, sampler): {sorted(vgprs.items())}")
    assert found == {(t, i) for t in range(2) for i in range(3)}, sorted(found)
