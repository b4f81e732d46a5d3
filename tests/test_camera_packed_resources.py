"""The packed camera kernels own no scratch memory, and of LDS what DESIGN.md section 21 states: tools/isa_kernels.py over the
built objects reports `scratch 0` and `vgpr spilled 0` for every compose_cam_packed_kernel<OutLens, Interp, CH, Fmt> and
cam_overlap_packed_kernel<OutLens, Fmt>; `lds` 2048 (both 8-bit tables) for a compose kernel of 8-bit frames and 1024 (the
thresholds alone) for one of half frames; `lds` 12288 + 1024 (the decode table) for a statistic kernel of 8-bit frames and 12288
for one of half frames.  The instantiations are exactly 5 output lenses x 3 samplers x {run-time channels, RGBA} x {half, 8-bit}
and 5 output lenses x {half, 8-bit}.  Resource figures only; no instruction text is read.  Skipped when the objects are not
built."""
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "image-lens-reproject_amd", "lib", "obj")
COMPOSE = re.compile(r"^_ZN3lrp\d+compose_cam_packed_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEEvNS_\d+CameraPackedParamsE$")
STAT = re.compile(r"^_ZN3lrp\d+cam_overlap_packed_kernelILi(\d+)ELi(\d+)EEEvNS_\d+CameraStatPackedParamsE$")
F16, U8 = 1, 2


def _kernels(tmp_path, pattern, at_least):
    units = sorted(glob.glob(os.path.join(OBJ, pattern)))
    if len(units) < at_least:
        pytest.skip("the kernel objects are not built")
    for u in units:  # (the tool takes a directory: one with these units alone, not the whole build)
        os.symlink(u, tmp_path / os.path.basename(u))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_kernels.py"), "kernels", str(tmp_path)], check=True, capture_output=True,
                         text=True).stdout
    for line in out.splitlines():
        f = line.split()
        res = dict(zip(f[2::2], f[3::2]))  # sgpr N spilled N vgpr N spilled N lds N scratch N: the second `spilled` is the VGPRs'
        yield line, f[0], res, f[f.index("vgpr") + 3]


def _check(tmp_path, pattern, at_least, regex, name, lds_of):
    found, worst = set(), 0
    for line, symbol, res, vgpr_spilled in _kernels(tmp_path, pattern, at_least):
        m = regex.match(symbol)
        if not m:
            assert name not in symbol, f"a kernel of another signature: {symbol}"
            continue
        key = tuple(int(g) for g in m.groups())
        assert res["scratch"] == "0" and vgpr_spilled == "0", line
        assert int(res["lds"]) == lds_of(key[-1]), line
        worst = max(worst, int(res["vgpr"]))
        assert key not in found, line
        found.add(key)
    print(f"{len(found)} kernels; most VGPRs {worst}")
    return found


def test_compose_kernels_have_no_scratch_and_the_tables_of_lds(tmp_path):
    found = _check(tmp_path, "lrp_camera_packed*.o", 4, COMPOSE, "compose_cam_packed_kernel", lambda fmt: 2048 if fmt == U8 else 1024)
    assert found == {(o, i, c, f) for o in range(5) for i in range(3) for c in (0, 4) for f in (F16, U8)}, sorted(found)


def test_statistic_kernels_have_no_scratch_and_the_lds_of_the_reduction(tmp_path):
    found = _check(tmp_path, "lrp_camstat_packed.o", 1, STAT, "cam_overlap_packed_kernel", lambda fmt: 12288 + (1024 if fmt == U8 else 0))
    assert found == {(o, f) for o in range(5) for f in (F16, U8)}, sorted(found)
