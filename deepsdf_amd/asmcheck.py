"""Build-time check of the one place where inline asm leaves loads in flight across C++ code (dwstream.hpp dw_block_split).

The first asm statement of a step there issues 16 ``ds_read_b128`` (the raw A and B rows of the NEXT step) and ends without a
wait: all sixteen reads are in flight while four groups of MFMAs and cut instructions run; a second statement
(``s_waitcnt lgkmcnt(0)``) ends the window.  The compiler cannot see loads inside asm, so BETWEEN the two statements it believes
the 64 destination registers hold data: a copy, an AGPR move or a spill of one of them placed there would read stale registers.
Whether it does that is a register-allocation outcome -- so every build of the library (lab flags included) is checked on the
gfx950 code object itself:

  for each run of 16 ds_read_b128 whose statement leaves reads in flight: no instruction up to the next ``s_waitcnt lgkmcnt(0)``
  may name a destination VGPR of those reads, and none may touch scratch (a spill in the window).

Tooling only (no GPU, no torch): ``python -m deepsdf_amd.asmcheck [lib]``; deepsdf_amd.build runs it after every compile.
``python -m deepsdf_amd.asmcheck --same A B`` compares the instruction streams of two libraries, function by function (same_code).
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "dw_stream_split_kernel"


class AsmHazard(RuntimeError):
    pass


def tools_available():
    return all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"))


def extract_code_object(lib, out_dir):
    fat, co = os.path.join(out_dir, "fat.bin"), os.path.join(out_dir, "co.elf")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
    return co


def disassemble(co, name_part):
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
    names = sorted({f.split()[7] for f in syms.splitlines() if len(f.split()) >= 8 and f.split()[3] == "FUNC" and name_part in f.split()[7]})
    if len(names) != 1:
        raise AsmHazard(f"expected exactly one function matching {name_part!r} in the code object, found {names}")
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f"--disassemble-symbols={names[0]}", co],
                         capture_output=True, text=True, check=True).stdout
    ins = []
    for line in out.splitlines():
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//", line)
        if m:
            ins.append((m.group(1), m.group(2)))
    return ins


def vgprs(operands):
    """Set of VGPR numbers an operand string names: v7, v[4:7] (AGPRs a.. are a different file and do not count)."""
    regs = set()
    for m in re.finditer(r"(?<![a-z_0-9])v(\d+)(?![\d:\]])", operands):
        regs.add(int(m.group(1)))
    for m in re.finditer(r"(?<![a-z_0-9])v\[(\d+):(\d+)\]", operands):
        regs.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return regs


def check_split_wait_windows(ins):
    """Returns the number of windows checked; raises AsmHazard on a violation.  A window opens behind a run of 16 ds_read_b128
    (the fragment reads of dwstream.hpp) that is not closed by an ``s_waitcnt lgkmcnt(0)`` at once, and extends to the next
    ``s_waitcnt lgkmcnt(0)``: directly behind the reads either nothing (dw_block_split: all sixteen are in flight) or
    ``lgkmcnt(8)`` (the first eight have landed, the last eight are in flight: the first form of that block)."""
    windows = 0
    for i, (op, args) in enumerate(ins):
        if i < 16 or ins[i - 1][0] != "ds_read_b128" or op == "ds_read_b128":
            continue
        reads = ins[i - 16:i]
        if any(o != "ds_read_b128" for o, _ in reads):
            continue
        if op == "s_waitcnt" and "lgkmcnt(0)" in args:
            continue                       # reads and their wait in one statement: no window
        first_open = 8 if (op == "s_waitcnt" and "lgkmcnt(8)" in args) else 0
        in_flight = set()
        for _, a in reads[first_open:]:
            in_flight |= vgprs(a.split(",")[0])
        if len(in_flight) != 4 * (16 - first_open):
            raise AsmHazard(f"window at instruction {i}: the reads in flight name {len(in_flight)} destination VGPRs, "
                            f"expected {4 * (16 - first_open)}")
        start = i + 1 if first_open else i
        for j in range(start, len(ins)):
            o, a = ins[j]
            if o == "s_waitcnt" and "lgkmcnt(0)" in a:
                break
            if o.startswith("scratch_") or (o.startswith("buffer_") and "off" in a and "s[0:3]" in a):
                raise AsmHazard(f"scratch traffic inside the split-wait window: {o} {a}")
            hit = vgprs(a) & in_flight
            if hit:
                raise AsmHazard(f"instruction {j} inside the split-wait window names registers whose reads are still in flight "
                                f"(v{sorted(hit)}): {o} {a}")
            if o in ("s_endpgm", "s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz",
                     "s_cbranch_execz", "s_cbranch_execnz", "s_setpc_b64"):
                raise AsmHazard(f"control flow ({o}) inside the split-wait window before its s_waitcnt lgkmcnt(0)")
        else:
            raise AsmHazard("split-wait window is never closed by s_waitcnt lgkmcnt(0)")
        windows += 1
    return windows


def check_library(lib):
    """Raises AsmHazard if the library's dw_stream_split_kernel violates the rule or has no window at all; returns the number of
    windows found."""
    with tempfile.TemporaryDirectory(prefix="dsdf_asmcheck_") as d:
        ins = disassemble(extract_code_object(lib, d), KERNEL)
    n = check_split_wait_windows(ins)
    if n == 0:
        raise AsmHazard(f"{KERNEL}: no split-wait window found (16 ds_read_b128 left in flight); the check would be vacuous")
    return n


# ---- second audit: MFMA source registers overwritten by a later load (fused_bf16x8.hpp, two waves per SIMD) -----------------
# Measured on MI355X (profiles/r02_lab_bf16x8_race.log): with two waves per SIMD, a ds_read / buffer_load that the register
# allocator gave the registers an MFMA issued JUST BEFORE it reads as srcA / srcB produced run-to-run differences in 3 % of the
# rows.  The k-loop was rewritten so that a step's loads only replace what the PREVIOUS step consumed and are issued after the
# step's own MFMAs.  That is a property of the emitted code, so it is measured on the code object: for every load with a VGPR
# destination, the number of OTHER MFMAs issued between the last MFMA that reads one of those registers as srcA / srcB and the
# load, over every path (loop back-edges included).
def disassemble_with_addresses(co, name_part):
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
    names = sorted({f.split()[7] for f in syms.splitlines() if len(f.split()) >= 8 and f.split()[3] == "FUNC" and name_part in f.split()[7]})
    if len(names) != 1:
        raise AsmHazard(f"expected exactly one function matching {name_part!r} in the code object, found {names}")
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f"--disassemble-symbols={names[0]}", co],
                         capture_output=True, text=True, check=True).stdout
    return parse_listing(out)


def parse_listing(text):
    """llvm-objdump -d text of ONE function -> [dict(op, args, addr, target)] (target: the address a branch names, else None)."""
    base, ins = None, []
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <", line)
        if m and base is None:
            base = int(m.group(1), 16)
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line)
        if m:
            tgt = re.search(r"<[^>]*\+0x([0-9a-f]+)>", m.group(4))
            ins.append(dict(op=m.group(1), args=m.group(2), addr=int(m.group(3), 16),
                            target=(base + int(tgt.group(1), 16)) if tgt and base is not None else None))
    return ins


def mfma_src_reuse_distances(ins, limit=12, fall_through_only=False, edges=None):
    """{load index: MFMAs issued strictly between the last MFMA reading one of the load's destination VGPRs as srcA/srcB and
    the load} for every ds_read* / buffer_load* / global_load* with a VGPR destination that has such a reader within `limit`
    MFMAs on some path.  Which control-flow edges a path may follow (`edges`):
      "all"           fall-through and every branch edge: also contains paths the program's own guards exclude (a forward branch
                      over a block of MFMAs taken together with the branch that only a step WITH MFMAs takes);
      "loops"         fall-through and BACKWARD branch edges (target <= branch: loop back-edges) -- every conditional forward
                      branch not taken, every loop iterated: the steady state of a k-loop, where the loads at the top of the body
                      follow the last MFMAs of the previous trip;
      "fall_through"  fall-through edges alone (every conditional branch not taken; `fall_through_only=True` is the old name)."""
    if edges is None:
        edges = "fall_through" if fall_through_only else "all"
    if edges not in ("all", "loops", "fall_through"):
        raise ValueError(edges)
    by_addr = {x["addr"]: i for i, x in enumerate(ins)}
    preds = [[] for _ in ins]
    for i, x in enumerate(ins):
        uncond = x["op"] in ("s_branch", "s_endpgm", "s_setpc_b64")
        if i + 1 < len(ins) and not uncond:
            preds[i + 1].append(i)
        if edges != "fall_through" and x["op"].startswith(("s_branch", "s_cbranch")) and x["target"] in by_addr:
            if edges == "all" or x["target"] <= x["addr"]:
                preds[by_addr[x["target"]]].append(i)
    src_ab, acc_regs = {}, set()
    for i, x in enumerate(ins):
        if x["op"].startswith("v_mfma"):
            ops = [o.strip() for o in x["args"].split(",")]
            src_ab[i] = vgprs(ops[1]) | vgprs(ops[2])
            acc_regs |= vgprs(ops[0])
    out = {}
    for i, x in enumerate(ins):
        if not x["op"].startswith(("ds_read", "buffer_load", "global_load")) or " lds" in (" " + x["args"]):
            continue
        dest = vgprs(x["args"].split(",")[0])
        if not dest:
            continue
        best, seen, stack = None, set(), [(p, 0) for p in preds[i]]
        while stack:
            j, n = stack.pop()
            if (j, n) in seen or n > limit:
                continue
            seen.add((j, n))
            if j in src_ab:
                if src_ab[j] & dest:
                    best = n if best is None else min(best, n)
                    continue
                n += 1
            elif ins[j]["op"].startswith("v_") and vgprs(",".join(ins[j]["args"].split(",")[1:])) & acc_regs:
                continue          # a VALU instruction READING an MFMA result (epilogue arithmetic, bf8_drain's v_readfirstlane): it
                                  # completes only after the MFMA that writes the register, and the matrix pipe is in-order
            elif vgprs(ins[j]["args"].split(",")[0]) & dest and not ins[j]["op"].startswith(("v_cmp", "s_", "ds_write", "buffer_store", "global_store")):
                continue          # an earlier WRITER of the same register on this path: what it overwrote is no longer the MFMA's operand
            stack.extend((p, n) for p in preds[j])
        if best is not None:
            out[i] = best
    return out


def check_mfma_src_reuse(lib, kernel="fused_forward_bf16x8_kernel", min_distance=1):
    """Raises AsmHazard if, on a path of fall-through and loop back-edges (every loop iterated, no forward branch taken: the
    k-loop's steady state included), some load in `kernel` overwrites srcA/srcB registers of an MFMA with fewer than `min_distance`
    other MFMAs issued in between (the signature of the first 8-wave k-loop: 46 such loads; the rewritten loop: none);
    returns (smallest distance found, number of load/MFMA pairs looked at)."""
    with tempfile.TemporaryDirectory(prefix="dsdf_asmcheck_") as d:
        ins = disassemble_with_addresses(extract_code_object(lib, d), kernel)
    dist = mfma_src_reuse_distances(ins, edges="loops")
    if not dist:
        return None, 0
    worst = min(dist.values())
    if worst < min_distance:
        bad = [f"{ins[i]['op']} {ins[i]['args']} @ {ins[i]['addr']:#x} (distance {n})" for i, n in dist.items() if n < min_distance]
        raise AsmHazard(f"{kernel}: {len(bad)} load(s) overwrite MFMA source registers after fewer than {min_distance} other MFMAs: "
                        + "; ".join(bad[:4]))
    return worst, len(dist)


# ---- third audit: the register ring of dw_item<4> must keep rolling (dwstream.hpp, dw_stream_kernel) ------------------------------
# The fp32 dW loop prefetches DW_RING k-steps of 2 loads each into a ring of registers.  For four rounds its code object held ONE
# wait per revolution, ``s_waitcnt vmcnt(0)`` at the loop header: every load sat under a scalar branch, the compiler could not
# count outstanding loads across the back edge, and the wave drained the whole ring and sat through a memory round trip every
# DW_RING steps.  Nothing fails when that happens -- the results are the same -- so it is a property held on the code object:
# inside the steady-state loop of the full-width item every wait that names vmcnt leaves >= 2 (DW_RING - 2) loads in flight.
def innermost_loops(ins):
    """[(first, last)] instruction index ranges of the loops that contain no other loop: a backward branch and its target."""
    by_addr = {x["addr"]: i for i, x in enumerate(ins)}
    spans = sorted({(by_addr[x["target"]], i) for i, x in enumerate(ins)
                    if x["op"].startswith(("s_branch", "s_cbranch")) and x["target"] in by_addr and x["target"] <= x["addr"]})
    return [(a, b) for a, b in spans if not any((c, d) != (a, b) and a <= c and d <= b for c, d in spans)]


def dw_ring_waits(ins, ring):
    """The vmcnt values of every s_waitcnt inside the steady-state loop of dw_item<4>: THE innermost loop with 16 * ring MFMAs and
    2 * ring buffer loads (one revolution of the ring).  Raises AsmHazard if there is no such loop, or more than one."""
    found = []
    for a, b in innermost_loops(ins):
        body = ins[a:b + 1]
        if (sum(x["op"].startswith("v_mfma") for x in body) == 16 * ring
                and sum(x["op"].startswith("buffer_load") for x in body) == 2 * ring):
            found.append([int(m.group(1)) for x in body if x["op"] == "s_waitcnt" for m in re.finditer(r"vmcnt\((\d+)\)", x["args"])])
    if len(found) != 1:
        raise AsmHazard(f"dw ring: expected exactly one innermost loop of {16 * ring} MFMAs and {2 * ring} buffer loads "
                        f"(one revolution of a ring of {ring}), found {len(found)}; the check would be vacuous")
    return found[0]


def check_dw_ring_waits_ins(ins, ring):
    waits = dw_ring_waits(ins, ring)
    need = 2 * (ring - 2)
    if 0 in waits:
        raise AsmHazard(f"dw ring: s_waitcnt vmcnt(0) inside the steady-state loop (waits: {waits}): the ring is drained every revolution")
    if not waits or min(waits) < need:
        raise AsmHazard(f"dw ring: the steady-state loop's waits {waits} must all leave >= {need} loads in flight "
                        f"(2 * (DW_RING - 2), DW_RING = {ring})")
    return waits


def check_dw_ring_waits(lib, ring=16, kernel="dw_stream_kernel"):
    """Raises AsmHazard unless every vmcnt wait in the steady-state loop of `kernel` allows >= 2 (ring - 2) outstanding loads
    (and none is vmcnt(0)); returns the loop's wait counts in program order."""
    with tempfile.TemporaryDirectory(prefix="dsdf_asmcheck_") as d:
        ins = disassemble_with_addresses(extract_code_object(lib, d), kernel)
    return check_dw_ring_waits_ins(ins, ring)


# ---- comparing two libraries: has a source change moved any instruction? ---------------------------------------------------------
# A refactor of the kernel sources that must not change what the GPU executes is proved here, without a GPU: every function of
# the two gfx950 code objects is disassembled and compared as text, mnemonic and operands, in order.  ONE thing is masked: the
# literal of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64.  That is the PC-relative distance to data, and it moves in
# kernels nobody touched when code elsewhere in the translation unit changes size.
def function_streams(lib):
    """{name: [(mnemonic, operands)]} for every FUNC symbol of the library's gfx950 code object."""
    with tempfile.TemporaryDirectory(prefix="dsdf_asmcheck_") as d:
        co = extract_code_object(lib, d)
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    funcs = {f.split()[7]: [] for f in syms.splitlines() if len(f.split()) >= 8 and f.split()[3] == "FUNC"}
    cur = None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = funcs.get(m.group(1))
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//", line)
        if m and cur is not None:
            cur.append((m.group(1), m.group(2)))
    return funcs


def mask_pc_relative(ins):
    out = list(ins)
    for i in range(len(out) - 2):
        if out[i][0] == "s_getpc_b64" and out[i + 1][0] == "s_add_u32" and out[i + 2][0] == "s_addc_u32":
            for j in (i + 1, i + 2):
                out[j] = (out[j][0], out[j][1].rsplit(",", 1)[0] + ", <pc-relative>")
    return out


def same_streams(a, b):
    """a, b: {function: [(mnemonic, operands)]}.  Returns ({function in both: (instructions in a, instructions in b, index of the
    first difference or None)}, names only in a, names only in b)."""
    per = {}
    for name in sorted(set(a) & set(b)):
        x, y = mask_pc_relative(a[name]), mask_pc_relative(b[name])
        diff = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), None)
        if diff is None and len(x) != len(y):
            diff = min(len(x), len(y))
        per[name] = (len(x), len(y), diff)
    return per, sorted(set(a) - set(b)), sorted(set(b) - set(a))


def same_code(lib_a, lib_b):
    """same_streams of the gfx950 code objects of two builds of the library."""
    return same_streams(function_streams(lib_a), function_streams(lib_b))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--same"]:
        per, only_a, only_b = same_code(sys.argv[2], sys.argv[3])
        for name, (na, nb, diff) in per.items():
            print(f"{name} {na} " + ("equal" if diff is None else f"DIFFERENT at instruction {diff} ({na} / {nb} instructions)"))
        for name in only_a + only_b:
            print(f"{name} - ONLY IN {'A' if name in only_a else 'B'}")
        bad = sum(d is not None for _, _, d in per.values()) + len(only_a) + len(only_b)
        print(f"# {len(per)} functions compared, {bad} different or missing")
        sys.exit(1 if bad else 0)
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdsdf_hip.so")
    print(f"{KERNEL}: {check_library(lib)} split-wait window(s) clean")
