#!/usr/bin/env python3
"""Per-kernel view of the gfx950 code in a directory of objects (the per-kernel modes of tools/isa_hash.sh).

  isa_kernels.py kernels <obj-dir>          one line per kernel symbol, sorted:
                                            <symbol> <hash> sgpr N spilled N vgpr N spilled N lds N scratch N <object>
  isa_kernels.py compare <dir-a> <dir-b>    the kernels of b against those of a: added, lost, present in two objects,
                                            different in hash or resources; exit status 1 if any

The hash is of the kernel's disassembly without addresses, encodings and comments.  Branch operands are relative; the one
position-dependent operand, the literal of an s_getpc_b64 / s_add_u32 / s_addc_u32 address computation, is replaced by the
symbol it points to (+ offset).  So the hash does not depend on where in which object a kernel lies: one that moved
between units keeps its line but for the last field.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object of a host object, or None for a host-only one."""
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.devnull], capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}", "--unbundle"],
                   check=True, capture_output=True)
    return co


def address_symbols(co):
    """(address, size, name) of what an address computation may point to: data objects (kernel descriptors excluded) and
    functions (a branch beyond the reach of s_branch goes through s_getpc_b64 / s_setpc_b64)."""
    out = []
    for line in run(f"{LLVM}/llvm-readelf", "-s", "-W", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("OBJECT", "FUNC") and not f[7].endswith(".kd"):
            out.append((int(f[1], 16), int(f[2]), f[7]))
    return out


def kernel_texts(co):
    """symbol -> position-independent text."""
    syms = address_symbols(co)

    def name_of(addr):
        for a, n, s in syms:
            if a <= addr < a + max(n, 1):
                return f"<{s}+{addr - a}>"
        return f"<?{addr:#x}>"

    texts, cur, pc = {}, None, {}  # pc: low register of a pending s_getpc_b64 -> (address of the next instruction, high register)
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^<(.*)>:$", line)
        if m:
            cur, pc = texts.setdefault(m.group(1), []), {}
            continue
        if cur is None or not line.strip():
            continue
        text, _, comment = line.partition("//")
        text = text.strip()
        m = re.match(r"s_getpc_b64 (s\[(\d+):\d+\]|vcc)$", text)
        if m:
            lo, hi = ("vcc_lo", "vcc_hi") if m.group(1) == "vcc" else (f"s{m.group(2)}", f"s{int(m.group(2)) + 1}")
            pc[lo] = (int(comment.split(":")[0], 16) + 4, hi)
        else:
            m = re.match(r"(s_addc?_u32) (\w+), (\w+), (0x[0-9a-f]+|-?\d+)$", text)
            if m and m.group(2) == m.group(3) and m.group(2) in pc:
                if m.group(1) == "s_add_u32":
                    at, hi = pc.pop(m.group(2))
                    lit = int(m.group(4), 0) & 0xFFFFFFFF
                    target = (at + lit - (1 << 32 if lit >> 31 else 0)) & 0xFFFFFFFFFFFFFFFF
                    text = f"s_add_u32 {m.group(2)}, {m.group(2)}, {name_of(target)}@lo"
                    pc[hi] = None  # the s_addc_u32 of the high half follows
                elif pc.pop(m.group(2)) is None:
                    text = f"s_addc_u32 {m.group(2)}, {m.group(2)}, @hi"
        cur.append(text)
    return {k: "\n".join(v) for k, v in texts.items()}


def kernel_resources(co):
    """symbol -> resource line, from the metadata note."""
    res, cur = {}, {}
    keys = {".group_segment_fixed_size:": "lds", ".private_segment_fixed_size:": "scratch", ".sgpr_count:": "sgpr",
            ".sgpr_spill_count:": "sspill", ".vgpr_count:": "vgpr", ".vgpr_spill_count:": "vspill", ".name:": "name"}
    for line in run(f"{LLVM}/llvm-readelf", "--notes", co).splitlines():
        f = line.replace("- .", "  .").split()
        if len(f) == 2 and f[0] in keys:
            if f[0] == ".group_segment_fixed_size:":  # (the first key of a kernel's record that is read here)
                cur = {}
            cur[keys[f[0]]] = f[1]
            if len(cur) == len(keys):
                res[cur["name"]] = "sgpr {sgpr} spilled {sspill} vgpr {vgpr} spilled {vspill} lds {lds} scratch {scratch}".format(**cur)
    return res


def kernels(obj_dir):
    """[(symbol, hash + resources, object)], sorted."""
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(os.listdir(obj_dir)):
            if not name.endswith(".o"):
                continue
            co = code_object(os.path.join(obj_dir, name), tmp)
            if co is None:
                continue
            texts = kernel_texts(co)
            for sym, res in kernel_resources(co).items():
                rows.append((sym, hashlib.sha256(texts[sym].encode()).hexdigest()[:16] + " " + res, name))
    return sorted(rows)


def unique(rows, label):
    seen, bad = {}, 0
    for sym, what, obj in rows:
        if sym in seen:
            print(f"in two objects of {label}: {sym} ({seen[sym][1]}, {obj})")
            bad = 1
        seen[sym] = (what, obj)
    return seen, bad


def main(argv):
    if len(argv) == 3 and argv[1] == "kernels":
        for row in kernels(argv[2]):
            print(*row)
        return 0
    if len(argv) == 4 and argv[1] == "compare":
        a, bad_a = unique(kernels(argv[2]), "a")
        b, bad_b = unique(kernels(argv[3]), "b")
        bad, differ, moved = bad_a | bad_b, 0, 0
        for sym in sorted(set(a) | set(b)):
            if sym not in b:
                print("lost:", sym)
            elif sym not in a:
                print("added:", sym)
            elif a[sym][0] != b[sym][0]:
                print(f"differs: {sym}\n  a: {a[sym][0]}\n  b: {b[sym][0]}")
                differ += 1
            else:
                moved += a[sym][1] != b[sym][1]
                continue
            bad = 1
        print(f"kernels: {len(a)} in a, {len(b)} in b; {differ} differ; {moved} unchanged in another object")
        return bad
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
