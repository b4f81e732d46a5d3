#!/usr/bin/env python3
"""Per-kernel view of the gfx950 code in a directory of objects (the per-kernel modes of tools/isa_hash.sh).

  isa_kernels.py kernels <obj-dir>          one line per kernel symbol, sorted:
                                            <symbol> <hash> sgpr N spilled N vgpr N spilled N lds N scratch N <object>
  isa_kernels.py compare <dir-a> <dir-b>    the kernels of b against those of a: added, lost, present in two objects,
                                            different in hash or resources; exit status 1 if any
  isa_kernels.py passes <obj-dir> <symbol>  the coefficient-tier and raw-tap pass bodies of the window kernel <symbol> (a
                                            substring of its mangled name): per body its tier, ds_read_b128, packed and
                                            non-packed VALU instructions up to the global_store_dwordx4 (coef_passes below)

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


def kernel_listing(co, symbol):
    """[(address, text)] of the one kernel whose name contains `symbol`; None if there is none or more than one."""
    found, cur = {}, None
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^<(.*)>:$", line)
        if m:
            cur = found.setdefault(m.group(1), []) if symbol in m.group(1) and not m.group(1).endswith(".kd") else None
            continue
        if cur is None or not line.strip():
            continue
        text, _, comment = line.partition("//")
        m = re.match(r"\s*([0-9a-fA-F]+):", comment)
        if m and text.strip():
            cur.append((int(m.group(1), 16), text.strip()))
    return next(iter(found.values())) if len(found) == 1 else None


def coef_passes(listing):
    """The pass bodies of a window kernel that read their taps from the LDS window, in code order:
    [{"tier", "ds_read_b128", "packed", "valu", "lines", "valu_text"}], tier "coef" (coefficient tier) or "raw" (raw taps).

    The kernel's branches are structurized (a tier's code ends in flag tests, the tiers join in front of the store), so a
    body is told by what it holds, as two stretches of the code:
      * the tier's own.  It is found by its READ GROUP: 16 ds_read_b128 with nothing between them but address adds, the
        weights' multiplies, moves, scalar instructions and waits — in the last pass of the coefficient tier 4 + 12 with the
        request of the next window (global_load_lds_*) between them (precompute()'s groups of 4 or 8 reads in front of
        passes 0 and 2 are not one).  It begins behind the previous global_store_dwordx4, unconditional branch, loop end (a backward
        branch) or arithmetic / LDS access of another stretch, and runs through the reads (in the last pass the request of
        the next window lies behind them) and at least 82 v_pk_* to the branch that ends that block.  82-119 v_pk_*: the
        coefficient tier (four taps + twelve coefficient vectors, 82 for the cubics + 2 for 0.0f + s); 120 and more: raw
        taps (sixteen taps, five full cubics: 170);
      * the store's: the basic block of the next global_store_dwordx4 up to it — where the tiers join behind the tonemap,
        which a launch without post-processing branches over.
    `valu` counts the vector ALU instructions of the two that are not packed (v_* but not v_pk_*): what a pass issues beside
    its arithmetic — addresses, weights, flags.  Not counted: the blocks of flag tests between a tier's closing branch and
    the store's block (no vector instruction in the kernels looked at, but it makes this count a lower one than a count over
    everything between two stores)."""
    at = {a: i for i, (a, _) in enumerate(listing)}
    n = len(listing)

    def target(i):
        a, t = listing[i]
        off = int(t.split()[-1])
        return at.get(a + 4 + 4 * (off - 65536 if off >= 32768 else off))

    def is_branch(t):
        return t.startswith(("s_cbranch", "s_branch", "s_setpc"))

    def is_valu(t):
        return t.startswith("v_") and not t.startswith("v_pk_") and not t.startswith("v_nop")

    def in_read_group(t):
        return t.startswith(("ds_read_b128", "v_add_u32", "v_mul_f32", "v_mov_b32", "s_")) and not is_branch(t) and not t.startswith("s_endpgm")

    leaders = {target(i) for i in range(n) if listing[i][1].startswith(("s_cbranch", "s_branch"))}
    bodies, i = [], 0
    while i < n:
        if not listing[i][1].startswith("ds_read_b128"):
            i += 1
            continue
        e = i  # the read group [i, e)
        while e < n and in_read_group(listing[e][1]):
            e += 1
        reads = sum(t.startswith("ds_read_b128") for _, t in listing[i:e])
        if reads == 4:  # the last pass: the four taps, the request of the next window (global_load_lds_*, a loop), the twelve vectors
            m = e
            while m < n and m - e < 100 and not listing[m][1].startswith(("ds_", "v_pk_", "global_store_", "s_endpgm")):
                m += 1
            if m < n and listing[m][1].startswith("ds_read_b128") and any(t.startswith("global_load_lds") for _, t in listing[e:m]):
                e2 = m
                while e2 < n and in_read_group(listing[e2][1]):
                    e2 += 1
                if sum(t.startswith("ds_read_b128") for _, t in listing[m:e2]) == 12:
                    reads, e = 16, e2
        if reads != 16:
            i = e
            continue
        first = i
        while first > 0:
            t = listing[first - 1][1]
            if t.startswith(("global_store_", "s_endpgm", "s_branch", "s_setpc", "ds_read", "ds_write", "v_pk_")):
                break
            if t.startswith("s_cbranch") and (target(first - 1) or 0) < first:
                break
            first -= 1
        j, packed, stored = e, 0, False
        while j < n:
            t = listing[j][1]
            packed += t.startswith("v_pk_")
            stored = t.startswith("global_store_dwordx4")
            if stored or t.startswith("s_endpgm") or (packed >= 82 and is_branch(t)):
                break
            j += 1
        if packed < 82 or j >= n:
            i = e
            continue
        own = [t for _, t in listing[first:j + 1]]
        tail = []
        if not stored:
            k = j + 1
            while k < n and not listing[k][1].startswith("global_store_dwordx4"):
                k += 1
            b = k
            while b > j + 1 and b not in leaders and not is_branch(listing[b - 1][1]):
                b -= 1
            tail = [t for _, t in listing[b:min(k, n - 1) + 1]]
        path = own + tail
        bodies.append({"tier": "coef" if packed < 120 else "raw", "ds_read_b128": sum(t.startswith("ds_read_b128") for t in path),
                       "packed": sum(t.startswith("v_pk_") for t in path), "valu": sum(is_valu(t) for t in path), "lines": len(path),
                       "valu_text": [t for t in path if is_valu(t)]})
        i = j + 1
    return bodies


def kernel_passes(obj_dir, symbol, only=None):
    """coef_passes of the kernel whose mangled name contains `symbol`, searched in the objects of obj_dir (`only`: in these
    objects); None: not found."""
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(os.listdir(obj_dir)):
            if not name.endswith(".o") or (only is not None and name not in only):
                continue
            co = code_object(os.path.join(obj_dir, name), tmp)
            if co is None:
                continue
            listing = kernel_listing(co, symbol)
            if listing:
                return coef_passes(listing)
    return None


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
    if len(argv) == 4 and argv[1] == "passes":
        bodies = kernel_passes(argv[2], argv[3])
        if bodies is None:
            print("no such kernel:", argv[3])
            return 1
        for k, b in enumerate(bodies):
            print(f"pass body {k} ({b['tier']}): ds_read_b128 {b['ds_read_b128']} packed {b['packed']} non-packed VALU {b['valu']} instructions {b['lines']}")
            for t in b["valu_text"]:
                print("   ", t)
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
