#!/usr/bin/env python3
"""Per-kernel view of the gfx950 code in a directory of objects (the per-kernel modes of tools/isa_hash.sh).

  isa_kernels.py kernels <obj-dir>          one line per kernel symbol, sorted:
                                            <symbol> <hash> sgpr N spilled N vgpr N spilled N lds N scratch N <object>
  isa_kernels.py compare <dir-a> <dir-b>    the kernels of b against those of a: added, lost, present in two objects,
                                            different in hash or resources (with the instruction counts of both sides);
                                            exit status 1 if any
  isa_kernels.py passes <obj-dir> <symbol>  the coefficient-tier and raw-tap pass bodies of the window kernel <symbol> (a
                                            substring of its mangled name): per body its tier, ds_read_b128, packed and
                                            non-packed VALU instructions up to the global_store_dwordx4 (coef_passes below)
  isa_kernels.py frame <obj-dir> <symbol> [--rows N] [--trips M] [--half] [--post]
                                            the instructions of ONE FRAME of the coefficient-tier frame loop of a one-block
                                            window kernel, by class: packed, other VALU, LDS, vector memory, scalar, waits,
                                            branches; the request loop counted for N window rows, precompute() for M trips
                                            (coef_frame below)

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
                       "valu_text": [t for t in path if is_valu(t)], "span": (first, j)})
        i = j + 1
    return bodies


CLASSES = ("packed", "other VALU", "LDS", "vector memory", "scalar", "waits", "branches")


def instruction_class(t):
    if t.startswith("v_pk_"):
        return "packed"
    if t.startswith("v_"):
        return "other VALU"
    if t.startswith("ds_"):
        return "LDS"
    if t.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vector memory"
    if t.startswith(("s_waitcnt", "s_nop")):
        return "waits"
    if t.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm")):
        return "branches"
    return "scalar"


def coef_frame(listing, rows=12, trips=1, whole=True, post=False):
    """The instructions one wavefront issues for ONE FRAME of a block of the coefficient tier in a one-block frame-loop window
    kernel, by class (CLASSES) — a static account of the code, made the same way for every build:

      * the frame loop is the innermost loop (a backward branch and its target) around the four coefficient-tier pass bodies
        of coef_passes();
      * inside it, every loop (the merged spans of the backward branches) that writes coefficient planes (ds_write_b128) is a
        precompute() trip loop and counts `trips` times; the loop that requests window rows (global_load_lds_*) counts
        rows / (requests per trip) times.  A precompute() trip is counted with both of its chunks of 64 origins and the
        tests around them;
      * left out: what a FORWARD branch skips when the skipped span holds nothing of the coefficient path — no part of a
        coefficient-tier body, no precompute() loop: the bodies of the other tiers and the flag tests between them,
        where the tier is tested per pass, a corner block's stores; the tonemap (a span of arithmetic with v_div_scale_f32
        and no memory instruction) unless `post` — also where it is not skipped by a forward branch but lies behind a
        conditional latch of the frame loop, as the fall-through that ends in a latch of its own; with `whole`
        (planes of the whole block) the second precompute() and what is skipped with it; with an even `rows` the single row
        requested in front of a loop that requests rows in pairs (the span skipped behind an s_bitcmp0_b32).
    What is neither multiplied nor left out counts once.  -> ({class: count}, {"loop": (first, last), "left_out": n, ...}) or
    None when the kernel has no four coefficient-tier bodies inside one loop."""
    at = {a: i for i, (a, _) in enumerate(listing)}
    n = len(listing)
    text = [t for _, t in listing]

    def target(i):
        off = int(text[i].split()[-1])
        return at.get(listing[i][0] + 4 + 4 * (off - 65536 if off >= 32768 else off))

    coef = [b["span"] for b in coef_passes(listing) if b["tier"] == "coef"]
    if len(coef) != 4:
        return None
    branches = [(i, target(i)) for i in range(n) if text[i].startswith(("s_cbranch", "s_branch"))]
    branches = [(i, t) for i, t in branches if t is not None]
    first_body, last_body = coef[0][0], coef[-1][1]
    around = [(i, t) for i, t in branches if t <= first_body and i >= last_body]
    if not around:
        return None
    head = max(t for _, t in around)
    latches = [(i, t) for i, t in around if t > head - 32]  # (a structurized loop may close through two branches to neighbouring blocks)
    lo, hi = min(t for _, t in latches), max(i for i, _ in latches)
    # inner loops: merged spans of the backward branches inside the frame loop
    spans = sorted((t, i) for i, t in branches if lo < t <= i < hi and not (t <= first_body and i >= last_body))
    loops = []
    for t, i in spans:
        if loops and t <= loops[-1][1]:
            loops[-1][1] = max(loops[-1][1], i)
        else:
            loops.append([t, i])
    weight = [1] * n
    pre_loops = []
    for t, i in loops:
        body = text[t:i + 1]
        if any(x.startswith("global_load_lds") for x in body) and any(a <= t and i <= b for a, b in coef):  # (the request of a coefficient-tier pass)
            per_trip = sum(x.startswith("global_load_lds") for x in body)
            for k in range(t, i + 1):
                weight[k] = rows // per_trip
        elif sum(x.startswith("ds_write_b128") for x in body) >= 3:
            pre_loops.append((t, i))
            for k in range(t, i + 1):
                weight[k] = trips
    hot = [False] * n  # part of the coefficient path for certain
    for a, b in coef + pre_loops:
        for k in range(a, b + 1):
            hot[k] = True
    left_out = [False] * n
    for i, t in branches:
        if not (lo <= i < t <= hi + 1):
            continue
        skipped = range(i + 1, t)
        cold = not any(hot[k] for k in skipped)
        if cold and any(text[k].startswith("v_div_scale_f32") for k in skipped) and not any(text[k].startswith(("ds_", "global_")) for k in skipped):
            cold = not post  # the tonemap alone: arithmetic between a pass's sample and its store
        second = whole and len(pre_loops) >= 2 and any(pre_loops[1][0] <= k <= pre_loops[1][1] for k in skipped) and \
            not any(a <= k <= b for a, b in coef for k in skipped)
        odd_row = rows % 2 == 0 and i > 0 and text[i - 1].startswith("s_bitcmp0_b32") and any(text[k].startswith("global_load_lds") for k in skipped)
        if cold or second or odd_row:
            for k in skipped:
                left_out[k] = True
    # The loop may close through a CONDITIONAL latch with the tonemap of the last pass as its fall-through, ending in a latch
    # of its own (the parent of the per-tier loop: pass 3 without a tonemap branches back, the tonemap follows): no forward
    # branch skips that body, the latch in front of it does.
    order = sorted(i for i, _ in latches)
    for a, b in zip(order, order[1:]):
        body = range(a + 1, b + 1)
        if not post and text[a].startswith("s_cbranch") and any(text[k].startswith("v_div_scale_f32") for k in body) and \
                not any(hot[k] or text[k].startswith(("ds_", "global_")) for k in body):
            for k in body:
                left_out[k] = True
    counts = {c: 0 for c in CLASSES}
    for k in range(lo, hi + 1):
        if not left_out[k]:
            counts[instruction_class(text[k])] += weight[k]
    info = {"loop": (lo, hi), "static": hi - lo + 1, "left_out": sum(left_out[lo:hi + 1]), "precompute_loops": len(pre_loops),
            "rows": rows, "trips": trips, "whole": whole, "post": post}
    return counts, info


def kernel_frame(obj_dir, symbol, only=None, **kw):
    """coef_frame of the kernel whose mangled name contains `symbol`; None: not found, or no coefficient-tier loop in it."""
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(os.listdir(obj_dir)):
            if not name.endswith(".o") or (only is not None and name not in only):
                continue
            co = code_object(os.path.join(obj_dir, name), tmp)
            if co is None:
                continue
            listing = kernel_listing(co, symbol)
            if listing:
                return coef_frame(listing, **kw)
    return None


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
    """[(symbol, hash + resources, object, instructions)], sorted."""
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
                rows.append((sym, hashlib.sha256(texts[sym].encode()).hexdigest()[:16] + " " + res, name, len(texts[sym].splitlines())))
    return sorted(rows)


def unique(rows, label):
    seen, bad = {}, 0
    for sym, what, obj, count in rows:
        if sym in seen:
            print(f"in two objects of {label}: {sym} ({seen[sym][1]}, {obj})")
            bad = 1
        seen[sym] = (what, obj, count)
    return seen, bad


def main(argv):
    if len(argv) == 3 and argv[1] == "kernels":
        for row in kernels(argv[2]):
            print(*row[:3])
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
    if len(argv) >= 4 and argv[1] == "frame":
        import argparse
        ap = argparse.ArgumentParser(prog="isa_kernels.py frame")
        ap.add_argument("obj_dir")
        ap.add_argument("symbol")
        ap.add_argument("--rows", type=int, default=12, help="rows of the window (requests of the next frame's window)")
        ap.add_argument("--trips", type=int, default=1, help="trips of a precompute() loop (128 origins each)")
        ap.add_argument("--half", action="store_true", help="half-block planes: the second precompute() runs")
        ap.add_argument("--post", action="store_true", help="the tonemap runs")
        a = ap.parse_args(argv[2:])
        r = kernel_frame(a.obj_dir, a.symbol, rows=a.rows, trips=a.trips, whole=not a.half, post=a.post)
        if r is None:
            print("no such kernel, or no loop around four coefficient-tier bodies:", a.symbol)
            return 1
        counts, info = r
        print(f"frame loop: instructions {info['loop'][0]}..{info['loop'][1]} of the kernel ({info['static']} static, {info['left_out']} left out), "
              f"{info['precompute_loops']} precompute() loops; rows {a.rows}, trips {a.trips}, {'half' if a.half else 'whole'}-block planes, tonemap {'on' if a.post else 'off'}")
        for c in CLASSES:
            print(f"  {c:14s} {counts[c]:5d}")
        print(f"  {'per frame':14s} {sum(counts.values()):5d}   per pass {sum(counts.values()) / 4:.1f}")
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
                print(f"differs: {sym}\n  a: {a[sym][0]} instructions {a[sym][2]}\n  b: {b[sym][0]} instructions {b[sym][2]}")
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
