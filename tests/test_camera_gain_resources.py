"""The exposure-matching kernels: tools/isa_kernels.py over the built objects reports `scratch 0` and
`vgpr spilled 0` for all of them; `lds 0` for every camgain_kernel<OutLens, Interp> — exactly 5 output lenses x 3 samplers — and
the 12288 bytes the design states (q parked per lane, 8 x 256 x 4 bytes, and the four waves' tables, 4 x 128 x 8 bytes) for
every cam_overlap_kernel<OutLens> — exactly 5.  Resource
figures only; no instruction text is read.  Skipped when the objects are not built."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj")
GAIN = re.compile(r"^_ZN3lrp\d+camgain_kernelILi(\d+)ELi(\d+)EEEvNS_\d+CameraGainParamsE$")
STAT = re.compile(r"^_ZN3lrp\d+cam_overlap_kernelILi(\d+)EEEvNS_\d+CameraStatParamsE$")
STAT_LDS = 8 * 256 * 4 + 4 * 128 * 8


def _kernels(tmp_path, pattern, want_units):
    units = sorted(glob.glob(os.path.join(OBJ, pattern)))
    if len(units) < want_units:
        pytest.skip("the kernel objects are not built")
    for u in units:  # (the tool takes a directory: one with these units alone, not the whole build)
        os.symlink(u, tmp_path / os.path.basename(u))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_kernels.py"), "kernels", str(tmp_path)], check=True, capture_output=True,
                         text=True).stdout
    for line in out.splitlines():
        f = line.split()
        res = dict(zip(f[2::2], f[3::2]))  # sgpr N spilled N vgpr N spilled N lds N scratch N: the second `spilled` is the VGPRs'
        yield line, f[0], res, f[f.index("vgpr") + 3]


def test_gain_kernels_have_no_scratch_and_no_lds(tmp_path):
    found, vgprs = set(), {}
    for line, name, res, vgpr_spilled in _kernels(tmp_path, "lrp_camgain*.o", 3):
        m = GAIN.match(name)
        if not m:
            assert "camgain_kernel" not in name and "compose_cam_kernel" not in name, f"a kernel of another signature: {name}"
            continue
        assert res["scratch"] == "0" and vgpr_spilled == "0" and res["lds"] == "0", line
        key = tuple(int(g) for g in m.groups())
        assert key not in found, line
        found.add(key)
        vgprs.setdefault(key[1], []).append(int(res["vgpr"]))
    print("VGPRs per sampler:", {i: (min(v), max(v)) for i, v in sorted(vgprs.items())})
    assert found == {(o, i) for o in range(5) for i in range(3)}, sorted(found)


def test_overlap_kernels_have_no_scratch_and_the_stated_lds(tmp_path):
    found, vgprs = set(), []
    for line, name, res, vgpr_spilled in _kernels(tmp_path, "lrp_camstat*.o", 1):
        m = STAT.match(name)
        if not m:
            assert "cam_overlap_kernel" not in name, f"a kernel of another signature: {name}"
            continue
        assert res["scratch"] == "0" and vgpr_spilled == "0" and int(res["lds"]) == STAT_LDS, line
        assert int(m.group(1)) not in found, line
        found.add(int(m.group(1)))
        vgprs.append(int(res["vgpr"]))
    print(f"{len(found)} kernels; VGPRs {min(vgprs)}-{max(vgprs)}")
    assert found == set(range(5)), sorted(found)
