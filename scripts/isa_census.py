#!/usr/bin/env python3
"""Static instruction census of the fused kernel's level loop (no GPU needed): what one wave issues per Gaussian level, by
category and by phase, for every blur radius of the default level table -- the audit of the PMC figure "VALU instructions per
computed pixel" (profiles/r05g_pmc_traffic.json: 2370 on band tiles, of which 1335 are the blur's executed flops).

    python scripts/isa_census.py [-DMST_...=...] [other_revision.hip [other_mst_diff.hip]] > profiles/r06_isa_census.txt

How: hipcc -S (device only, the product flags of mustache_amd/csrc/Makefile) on mst_scale_space.hip; the band-source kernel of
the default tile (Tile<32,64,14,8,1,false,false>, BAND = true) is cut into basic blocks with LLVM's own loop annotations
("in Loop: Header=... Depth=2" = the level loop).  Inside the loop a block that holds v_mul_f64 belongs to one case of the
radius switch: [axis-0 main items] -> [axis-0 leftover pieces, executed by the first 16 r threads only] -> s_barrier ->
[axis-1 pass]; the radius of a case follows from its multiplies (8 (r + 1) in the main block).  Everything else in the loop is
common to all radii: tap fetch, dispatch, DoG, edge strip, second barrier, 3 x 3 maximum, sieve, statistics, state moves.
Blocks of the branchy sieve form that only run when some lane passes a test are counted as executed (an upper bound).

The report ends with the inner tile's diagonal walk (mst_stage_walk.h) in the fused kernel and, beside it, in diff_dog_kernel's
band source (fused_walk(), diff_walk(); tests/test_stage_walk_census.py).

    python scripts/isa_census.py --window-loads [library.so] > profiles/<tag>_window_loads.txt

The second form reads a BUILT library (llvm-objdump, default mustache_amd/libmustache_hip.so) and prints, for every kernel that
includes mst_fir.h -- the fused kernel at every tile and source, the difference kernel -- and per radius case and pass (axis-0
main items, axis-0 leftover pieces, axis-1), the count of each LDS read opcode and the VALU that is not tap arithmetic.  A
window load that is not a ds_read_b128 runs at half the LDS rate (mst_fir.h, fir_chunk); tests/test_window_load_kinds.py
asserts through window_loads() that no pass holds a ds_read2_b64.

    python scripts/isa_census.py --state-copies [library.so]

The third form reads a built library too and prints, for every instantiation of the fused kernel, the register-pair copies one
thread issues per level and how many of them sit behind the radius switch; tests/test_level_state_copies.py asserts through
state_copies() that only the two renames of D and G are left."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "mustache_amd", "csrc", "mst_scale_space.hip")
FLAGS = ("-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Wno-unused-function -fno-honor-nans "
         "-mno-amdgpu-ieee --cuda-device-only -S").split()
KERNEL = re.compile(r"^_ZN\S*scale_space_kernelINS_4TileILi32ELi64ELi14ELi8ELi1ELb0ELb0EEELb1EEE\S*:")

CATS = ["fp64 add/mul", "fp64 max/min", "fp64 compare", "v_mov_b64", "v_mov_b32", "DPP move", "v_cndmask", "int / bit VALU",
        "int compare -> mask", "LDS read", "LDS write", "SALU", "s_waitcnt / s_nop", "branch", "barrier", "scalar load", "other"]
VALU = CATS[:9]


# Issue slots (one slot = the 4 cycles a SIMD takes to issue one FP64 instruction of a wave64), from the microbenchmarks of
# scripts/ubench (issue_mix.hip, f32_ops.hip; LABBOOK round 2): FP64 arithmetic, maxima, compares, DPP moves, v_mov_b64 and
# selects one slot; plain 32-bit integer VALU half a slot; a compare into a scalar mask that an s_or_b64 / s_and_b64 then
# folds into another mask 2.5 slots for an integer compare and its fold -- charged as half a slot for the compare and 2 for
# the scalar fold, whichever instruction wrote the masks; s_nop N stalls the wave's issue for N + 1 cycles.  Other scalar
# instructions, branches and waits are not charged.  v_addc_co_u32 / v_add_co_u32 are charged as the 32-bit integer adds
# they are (not timed on their own).  The table prices instructions in isolation: LABBOOK "Sieve gate" holds what the
# kernel's own timing says of it.
SLOTS = {"fp64 add/mul": 1.0, "fp64 max/min": 1.0, "fp64 compare": 1.0, "v_mov_b64": 1.0, "DPP move": 1.0, "v_cndmask": 1.0,
         "v_mov_b32": 0.5, "int / bit VALU": 0.5, "int compare -> mask": 0.5}
FOLD = 2.0


def is_fold(op, text):
    """a scalar and / or of two lane masks (not the exec bookkeeping of a branch)"""
    return op in ("s_or_b64", "s_and_b64") and "exec" not in text


def slots(ins):
    """issue slots of a list of (op, text)"""
    s = 0.0
    for op, text in ins:
        if op == "s_nop":
            s += (int(text.split()[1], 0) + 1) / 4.0
        elif is_fold(op, text):
            s += FOLD
        else:
            s += SLOTS.get(category(op, text), 0.0)
    return s


def category(op, text):
    if "dpp" in op or " row_" in text or " wave_sh" in text or "row_bcast" in text:
        return "DPP move"
    if op.startswith("v_cmp") and "f64" not in op and re.match(r"\S+\s+s\[", text):
        return "int compare -> mask"
    if op.startswith(("v_add_f64", "v_mul_f64", "v_fma_f64", "v_fmac_f64")):
        return "fp64 add/mul"
    if op.startswith(("v_max_f64", "v_min_f64")):
        return "fp64 max/min"
    if op.startswith("v_cmp") and "f64" in op:
        return "fp64 compare"
    if op.startswith("v_mov_b64"):
        return "v_mov_b64"
    if op.startswith(("v_mov_b32", "v_accvgpr")):
        return "v_mov_b32"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith("v_"):
        return "int / bit VALU"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "LDS read"
    if op.startswith("ds_"):
        return "LDS write"
    if op in ("s_waitcnt", "s_nop"):
        return "s_waitcnt / s_nop"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc")):
        return "branch"
    if op == "s_barrier":
        return "barrier"
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar load"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def kernel_text(defines, src=SRC, keep_files=False, kernel=KERNEL, flags=FLAGS):
    """the assembly lines of the default tile's band-source kernel; keep_files: with the file's .file directives in front"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + list(flags) + list(defines) + ["-I" + os.path.dirname(SRC), "-I" + os.path.join(ROOT, "include"),
                        src, "-o", out], check=True, capture_output=True)
        lines = open(out).read().split("\n")
    i0 = next(i for i, l in enumerate(lines) if kernel.match(l))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return ([l for l in lines if re.match(r"\s*\.file\s", l)] if keep_files else []) + lines[i0 + 1:i1]


def blocks(lines):
    """[(label, loop annotation, [(op, text)])] in layout order"""
    out, cur = [], ["entry", "", []]
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", l) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", l)
        if m:
            out.append(tuple(cur))
            cur = [m.group(1), m.group(2) or "", []]
            continue
        t = l.strip()
        if not t or t.startswith((";", ".")):
            if t.startswith(";") and "Loop" in t and not cur[2]:
                cur[1] += " " + t
            continue
        cur[2].append((t.split()[0], t))
    out.append(tuple(cur))
    return out


def count(ins):
    c = collections.Counter()
    for op, text in ins:
        c[category(op, text)] += 1
    return c


# ---- window loads per radius case and pass, from a BUILT library (llvm-objdump; tests/test_window_load_kinds.py) ----------
# Every blur kernel that includes mst_fir.h: the fused kernel (every tile, band and dense source) and the difference kernel.
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
LIB = os.path.join(ROOT, "mustache_amd", "libmustache_hip.so")
BLUR_KERNEL = re.compile(r"^[0-9a-f]+ <(_ZN\S*?(scale_space_kernel|diff_dog_kernel)I\S*)>:$")
TILE = re.compile(r"4TileILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])EEE?(.*)$")
INSN = re.compile(r"^\s+(\S+)\s*(.*?)\s*// ([0-9A-F]+):(?: [0-9A-F]{8})+(?: <[^>+]+\+0x([0-9a-f]+)>)?\s*$")
PASSES = ("axis-0 main", "axis-0 pieces", "axis-1")
PIECE_ROWS = 4      # vpass: rows per leftover piece


def kernel_title(name):
    """'scale_space_kernel Tile<32,64,14,8,1,0,0> band' from the mangled name"""
    m = TILE.search(name)
    base = "scale_space_kernel" if "scale_space_kernel" in name else "diff_dog_kernel"
    if base == "scale_space_kernel":
        src = "band" if m.group(8).startswith("Lb1E") else "dense"
    else:
        src = "band" if "BandSource" in m.group(8) else "dense"
    return "%s Tile<%s> %s source" % (base, ",".join(m.group(i) for i in range(1, 8)), src)


def disassemble(lib=LIB):
    """{mangled kernel name: [(address, op, text, branch target or None)]} of the blur kernels in a built library"""
    sys.path.append(os.path.dirname(os.path.abspath(__file__)))      # kernel_resources.py lies next to this file
    import kernel_resources
    out = {}
    for co in kernel_resources.code_objects(lib):
        txt = subprocess.run([OBJDUMP, "-d", co], check=True, capture_output=True, text=True).stdout
        cur = base = None
        for l in txt.split("\n"):
            if l and not l[0].isspace():
                m = BLUR_KERNEL.match(l)
                cur = out.setdefault(m.group(1), []) if m else None
                base = int(l.split()[0], 16) if m else None
                continue
            m = INSN.match(l) if cur is not None else None
            if m:
                cur.append((int(m.group(3), 16), m.group(1), m.group(1) + " " + m.group(2),
                            base + int(m.group(4), 16) if m.group(4) and m.group(1).startswith(("s_cbranch", "s_branch")) else None))
    return out


def disasm_blocks(ins):
    """basic blocks [[(op, text)]] in layout order: cut behind every branch, s_barrier, s_endpgm and in front of every branch target"""
    targets = {t for _, _, _, t in ins if t is not None}
    out, cur = [], []
    for addr, op, text, _ in ins:
        if addr in targets and cur:
            out.append(cur)
            cur = []
        cur.append((op, text))
        if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm")) or op == "s_barrier":
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def pass_blocks(ins, K):
    """{radius: (axis-0 main, axis-0 pieces, axis-1)}, each the block's [(op, text)].  A block that holds tap products belongs to a
    pass; a radius case is three such blocks in a row with K (r + 1), 4 (r + 1) and K (r + 1) products (multiplies, or multiply +
    fused multiply-adds in the FMA tiles)."""
    taps = lambda b: sum(1 for op, _ in b if op.startswith(("v_mul_f64", "v_fma_f64", "v_fmac_f64")))
    bl = [(b, taps(b)) for b in disasm_blocks(ins)]
    bl = [(b, n) for b, n in bl if n]
    cases, k = {}, 0
    while k + 2 < len(bl):
        n = bl[k][1]
        r = n // K - 1
        if n % K == 0 and r >= 1 and bl[k + 1][1] == PIECE_ROWS * (r + 1) and bl[k + 2][1] == n and r not in cases:
            cases[r] = (bl[k][0], bl[k + 1][0], bl[k + 2][0])
            k += 3
        else:
            k += 1
    return cases


def lds_reads(block):
    """Counter of the LDS read opcodes of a block"""
    return collections.Counter(op for op, _ in block if category(op, "") == "LDS read")


def other_valu(block):
    """VALU instructions of a pass block that are not tap arithmetic: address arithmetic and moves"""
    c = count(block)
    return sum(c[x] for x in VALU) - c["fp64 add/mul"]


def window_loads(lib=LIB):
    """[(title, RMAX, {radius: ((LDS read Counter, other VALU) per pass)})] for every blur kernel of the library"""
    res = []
    for name, ins in sorted(disassemble(lib).items(), key=lambda kv: kernel_title(kv[0])):
        m = TILE.search(name)
        cases = pass_blocks(ins, int(m.group(4)))
        res.append((kernel_title(name), int(m.group(3)), {r: tuple((lds_reads(b), other_valu(b)) for b in ps) for r, ps in cases.items()}))
    return res


def window_loads_report(lib):
    print("LDS reads and address arithmetic of the blur passes, per radius case, from %s" % os.path.relpath(lib, ROOT))
    print("per pass: count of each LDS read opcode; VALU that is not tap arithmetic (addresses, moves)")
    for title, rmax, cases in window_loads(lib):
        ops = sorted({op for ps in cases.values() for c, _ in ps for op in c})
        tot = collections.Counter()
        print()
        print("%s: radius cases found %d of %d" % (title, len(cases), rmax))
        print("   r  " + "".join("| %-*s" % (11 * len(ops) + 7, p) for p in PASSES))
        print("      " + "".join("| " + "".join("%-11s" % op[3:] for op in ops) + " VALU  " for _ in PASSES))
        for r in sorted(cases):
            print("  %2d  " % r + "".join("| " + "".join("%-11d" % c[op] for op in ops) + " %-6d" % v for c, v in cases[r]))
            for c, _ in cases[r]:
                tot.update(c)
        print("  all passes: " + ", ".join("%d %s" % (tot[op], op) for op in ops))


# ---- register-pair copies of the level loop, from a BUILT library (tests/test_level_state_copies.py) -------------------------
def is_pair_copy(op, text):
    """v_mov_b64 from a VGPR pair (not a constant load): a rename of per-pixel state, or a merge copy behind a join"""
    return op.startswith("v_mov_b64") and re.search(r",\s*v\[", text) is not None


def branch_edges(ins):
    """[(address, target)] of every branch of disassemble()'s instruction list; the long form (s_getpc_b64, s_add_u32, s_addc_u32,
    s_setpc_b64: the wide tile's kernel is longer than a 16-bit branch offset reaches) included"""
    out = []
    for i, (addr, op, text, target) in enumerate(ins):
        if target is not None:
            out.append((addr, target))
        elif op.startswith("s_setpc_b64") and i >= 3 and ins[i - 3][1].startswith("s_getpc_b64") and \
                ins[i - 2][1].startswith("s_add_u32") and ins[i - 1][1].startswith("s_addc_u32"):
            off = ((int(ins[i - 1][2].split(",")[-1], 0) & 0xffffffff) << 32) | (int(ins[i - 2][2].split(",")[-1], 0) & 0xffffffff)
            out.append((addr, ins[i - 3][0] + 4 + (off - (1 << 64) if off >= 1 << 63 else off)))
    return out


def state_copies(lib=LIB):
    """[(title, K, copies per level, copies behind the radius switch)] for every scale_space_kernel of the library.
    The level loop is the innermost loop around the radius cases: of the backward branches that enclose every tap product, those
    with the highest target.  Copies per level: the register-pair copies inside it (none lies in a radius case) -- with one
    static register assignment the floor is 2 K, one rename each of D and G (Dc = d, gprev = g).  Behind the switch: the copies
    between the last tap product and the first DoG subtraction, where the compiler merges the cases' accumulators into g if
    some path through the switch runs no case."""
    is_tap = lambda op: op.startswith(("v_mul_f64", "v_fma_f64", "v_fmac_f64"))
    res = []
    for name, ins in sorted(disassemble(lib).items(), key=lambda kv: kernel_title(kv[0])):
        if "scale_space_kernel" not in name:
            continue
        taps = [a for a, op, _, _ in ins if is_tap(op)]
        around = [(a, t) for a, t in branch_edges(ins) if t <= taps[0] and a >= taps[-1]]
        head = max(t for _, t in around)
        end = max(a for a, t in around if t == head)
        dog = next(a for a, op, text, _ in ins if a > taps[-1] and op.startswith("v_add_f64") and ", -v[" in text)
        copies = [a for a, op, text, _ in ins if is_pair_copy(op, text)]
        res.append((kernel_title(name), int(TILE.search(name).group(4)), sum(head <= a <= end for a in copies),
                    sum(taps[-1] < a < dog for a in copies)))
    return res


def state_copies_report(lib):
    print("register-pair copies (v_mov_b64 from a VGPR pair) of the fused kernel's level loop, from %s" % os.path.relpath(lib, ROOT))
    print("  per thread and level | behind the radius switch (of those)")
    for title, K, per_level, behind in state_copies(lib):
        print("  %-55s K = %d   %3d | %d" % (title, K, per_level, behind))


# ---- outside the level loop, by path (staging, tested mask, state initialisation, epilogue) -------------------------------------
# The kernel is compiled with line tables (-gline-tables-only: the instruction stream is the same, .loc directives are added)
# and every instruction outside the level loop is booked on the path whose source lines it comes from.  A path starts at its
# anchor line and ends at the next anchor: a "[census: <path>]" tag in a comment where the source has one, else the line that
# opens the path in the revisions without tags.  Instructions of inlined helpers (other files, or above the kernel) go with
# the instruction before them.
WALK_PATH = "staging: inner diagonal walk"
WALK_HEADER = "mst_stage_walk.h"      # the walk's body since round 11; the fused kernel calls it behind `} else if (inner) {`
EMPTY_PATH = "epilogue: empty workgroup"      # the short path of a workgroup without a tested pixel, where the source has one
PATHS = [
    ("prologue: work item, in_mask", [r"^scale_space_kernel\("]),
    ("staging: dense source", [r"if constexpr \(!BAND\) \{"]),
    ("staging: band setup, tile kind", [r"// ---- band source"]),
    ("staging: constant", [r"if \(constant\) \{"]),
    ("staging: inner diagonal walk", [r"\} else if \(inner\) \{"]),
    ("staging: border", [r"// border tiles"]),
    ("tested mask: build, count, any_nz", [r"uint32_t mine = 0;"]),
    ("state init, pass addresses", [r"// per-pixel rolling state"]),
    ("level loop: entry and exit", [r"for \(int o = 0; o < n_oct"]),
    ("epilogue: arguments", [r"// ---- found pixels"]),
    (EMPTY_PATH, [r"\[census: epilogue empty\]"]),
    ("epilogue: reservation", [r"\[census: epilogue reservation\]", r"uint32_t my_total = 0;"]),
    ("epilogue: statistics fold", [r"\[census: epilogue fold\]", r"for \(int t = tid; t < tested; t \+= T::NT\)"]),
    ("epilogue: record writes", [r"\[census: epilogue records\]", r"const uint32_t wave_base = "]),
]
KINDS = ("constant tile", "inner tile, tested", "border tile")
# Trips of a path's loops per tile kind, for the busiest wave of the default tile (CTR = 60, CTC = 92, CTP = 62, 256 threads, 4
# waves): constant 92 * 62 / 2 / 256 double2 stores; inner walk 151 diagonals in rounds of 4 waves x 19; border 60 * 92 / 256
# elements; every other loop outside the level loop runs once in the wave that runs it (the fold, the st slots, thread 0's scan).
LOOP_TRIPS = {"staging: constant": 92 * 62 / 2 / 256.0, "staging: inner diagonal walk": 2.0, "staging: border": 60 * 92 / 256.0}
STAGING_OF = {"staging: constant": KINDS[0], "staging: inner diagonal walk": KINDS[1], "staging: border": KINDS[2]}


def path_anchors(src):
    """[(first line, path)] in line order, and the kernel's (first, last) line, from the source text"""
    text = open(src).read().split("\n")
    k0 = next(i for i, l in enumerate(text) if l.startswith("scale_space_kernel(")) + 1
    k1 = next(i for i in range(k0, len(text)) if text[i].startswith("// partial[item][t][2]")) + 1
    out = []
    for path, alts in PATHS:
        for rx in alts:
            hit = next((i + 1 for i in range(k0 - 1, k1) if re.search(rx, text[i])), None)
            if hit:
                out.append((hit, path))
                break
    return sorted(out), (k0, k1)


def outside_by_path(lines, src, loop_labels, files):
    """{path: {"straight": Counter, "looped": Counter}} of the instructions outside the level loop; lines: kernel_text(..., line
    tables); loop_labels: the labels of the level loop's blocks; files: main_files(lines, src)"""
    anchors, (k0, k1) = path_anchors(src)
    res = collections.OrderedDict((p, {"straight": collections.Counter(), "looped": collections.Counter()}) for _, p in anchors)
    path, skip, looped, fresh = anchors[0][1], False, False, False
    walk_files = header_files(lines, WALK_HEADER)      # the walk's body lies in a header of its own: booked where it is called
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", l) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", l)
        if m:
            skip, looped, fresh = m.group(1) in loop_labels, "Loop" in (m.group(2) or ""), True
            continue
        t = l.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            if int(m.group(1)) in files and k0 <= int(m.group(2)) <= k1:
                path = [p for a, p in anchors if a <= int(m.group(2))][-1]
            elif int(m.group(1)) in walk_files and WALK_PATH in res:
                path = WALK_PATH
            continue
        if not t or t.startswith((";", ".")):
            if t.startswith(";") and "Loop" in t and fresh:
                looped = True
            continue
        fresh = False
        if not skip:
            res[path]["looped" if looped else "straight"][category(t.split()[0], t)] += 1
    return res


def header_files(lines, name):
    """the .file numbers that name a source file or header"""
    out = set()
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+(.*)$', l)
        if m and name in m.group(2):
            out.add(int(m.group(1)))
    return out


def main_files(lines, src):
    """the .file numbers that name the kernel's own source file"""
    return header_files(lines, os.path.basename(src))


# ---- the inner tile's diagonal walk (mst_stage_walk.h), in the fused kernel and in the difference kernel -------------------------
# Fused kernel: the path "staging: inner diagonal walk" of outside_by_path().  Difference kernel (mst_diff.hip, band source, the
# tile of the fused kernel's default radius): the instructions of the header and of the lines between `if (inner) {` and the
# `} else {` that closes it in BandSource::stage.  Weighted = straight + looped x rounds (busiest wave).
DIFF_SRC = os.path.join(ROOT, "mustache_amd", "csrc", "mst_diff.hip")
DIFF_FLAGS = [f for f in FLAGS if f not in ("-fno-honor-nans", "-mno-amdgpu-ieee")]
DIFF_KERNEL = re.compile(r"^_ZN\S*diff_dog_kernelINS_4TileILi32ELi64ELi14ELi8ELi1ELb0ELb0EEENS_10BandSourceEEE\S*:")
DIFF_ROUNDS = 4.0      # 38 diagonals per wave, 10 in flight (two loads each)


def walk_level_loop(bl):
    """(head label, blocks) of the level loop among blocks(): the depth-2 loop that holds barriers"""
    heads = collections.Counter()
    for lab, ann, ins in bl:
        m = re.search(r"Header=(BB\d+_\d+) Depth=2", ann)
        if m and any(op == "s_barrier" for op, _ in ins):
            heads[m.group(1)] += 1
    head = heads.most_common(1)[0][0]
    return head, [b for b in bl if re.search(r"(Header=%s Depth=2|Parent Loop %s)" % (head, head), b[1])]


def fused_walk(src=SRC, defines=()):
    """{"straight", "looped", "salu", "weighted"}: VALU per thread of the fused kernel's inner walk (default tile, band source),
    compiled from the source (tests/test_stage_walk_census.py)"""
    head, in_loop = walk_level_loop(blocks(kernel_text(defines, src)))
    located = kernel_text(list(defines) + ["-gline-tables-only"], src, keep_files=True)
    d = outside_by_path(located, src, {lab for lab, ann, ins in in_loop}, main_files(located, src))[WALK_PATH]
    valu = lambda c: sum(c[x] for x in VALU)
    s, lp = valu(d["straight"]), valu(d["looped"])
    return {"straight": s, "looped": lp, "salu": d["straight"]["SALU"] + d["looped"]["SALU"], "weighted": s + lp * LOOP_TRIPS[WALK_PATH]}


def diff_walk(src=DIFF_SRC):
    """the same figures for diff_dog_kernel's band source"""
    lines = kernel_text(["-gline-tables-only"], src, keep_files=True, kernel=DIFF_KERNEL, flags=DIFF_FLAGS)
    text = open(src).read().split("\n")
    a = next(i for i, l in enumerate(text) if re.search(r"^\s*if \(inner\) \{", l)) + 1
    b = next(i for i in range(a, len(text)) if re.match(r"^        \} else \{", text[i])) + 1
    # the element rule both of the source's paths share (the `pixel` lambda above them) goes with the instruction before it
    p0 = next(i for i, l in enumerate(text) if "auto pixel = " in l) + 1
    p1 = next(i for i in range(p0, len(text)) if re.match(r"^\s*\};", text[i])) + 1
    own, walk = main_files(lines, src), header_files(lines, WALK_HEADER)
    c = {"straight": collections.Counter(), "looped": collections.Counter()}
    inside, looped, fresh = False, False, False
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", l) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", l)
        if m:
            looped, fresh = "Loop" in (m.group(2) or ""), True
            continue
        t = l.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            f, ln = int(m.group(1)), int(m.group(2))
            if f in walk:
                inside = True
            elif f in own and not p0 <= ln <= p1:
                inside = a <= ln < b
            continue
        if not t or t.startswith((";", ".")):
            if t.startswith(";") and "Loop" in t and fresh:
                looped = True
            continue
        fresh = False
        if inside:
            c["looped" if looped else "straight"][category(t.split()[0], t)] += 1
    valu = lambda k: sum(k[x] for x in VALU)
    s, lp = valu(c["straight"]), valu(c["looped"])
    return {"straight": s, "looped": lp, "salu": c["straight"]["SALU"] + c["looped"]["SALU"], "weighted": s + lp * DIFF_ROUNDS}


def walk_report(src, defines, diff_src):
    print()
    print("the inner tile's diagonal walk, VALU per thread: straight-line | inside a loop | SALU | weighted by rounds (busiest wave)")
    f = fused_walk(src, defines)
    print("  %-58s %8d %7d %6d | %6.0f" % ("scale_space_kernel Tile<32,64,14,8,1,0,0> band source", f["straight"], f["looped"], f["salu"], f["weighted"]))
    if diff_src and not defines:
        d = diff_walk(diff_src)
        print("  %-58s %8d %7d %6d | %6.0f" % ("diff_dog_kernel Tile<32,64,14,8,1,0,0> band source", d["straight"], d["looped"], d["salu"], d["weighted"]))


def outside_report(res):
    valu = lambda c: sum(c[x] for x in VALU)
    has_empty_path = EMPTY_PATH in res      # path_anchors found its tag in the source
    print()
    print("outside the level loop by path, static VALU per thread: straight-line | inside a loop | SALU, and weighted by trip")
    print("count for three tile kinds (busiest wave; record writes with every pixel's branch taken = an upper bound; a path")
    print("that a kind does not run counts 0; the constant tile owns no tested pixel)")
    print("  %-36s %8s %7s %6s | %14s %19s %12s" % (("path", "straight", "looped", "SALU") + KINDS))
    tot = [0.0, 0.0, 0.0]
    tot_static = 0
    for path, d in res.items():
        s, lp = valu(d["straight"]), valu(d["looped"])
        if not s and not lp and not d["straight"]["SALU"] and not d["looped"]["SALU"]:
            continue
        w = []
        for kind in KINDS:
            if path in STAGING_OF:
                run = STAGING_OF[path] == kind
            elif path == EMPTY_PATH:
                run = kind == KINDS[0]
            elif path in ("epilogue: reservation", "epilogue: statistics fold", "epilogue: record writes"):
                run = not (has_empty_path and kind == KINDS[0])
            else:
                run = True
            w.append((s + lp * LOOP_TRIPS.get(path, 1.0)) if run else 0.0)
        tot = [a + b for a, b in zip(tot, w)]
        tot_static += s + lp
        print("  %-36s %8d %7d %6d | %14.0f %19.0f %12.0f" % (path, s, lp, d["straight"]["SALU"] + d["looped"]["SALU"], w[0], w[1], w[2]))
    print("  %-36s %8d %7s %6s | %14.0f %19.0f %12.0f" % ("all paths", tot_static, "", "", tot[0], tot[1], tot[2]))


def outside_valu(lib=LIB):
    """{title: static VALU instructions outside the level loop} for every scale_space_kernel of a BUILT library
    (tests/test_outside_loop_census.py).  The level loop as in state_copies(): the innermost loop around the radius cases."""
    is_tap = lambda op: op.startswith(("v_mul_f64", "v_fma_f64", "v_fmac_f64"))
    res = {}
    for name, ins in disassemble(lib).items():
        if "scale_space_kernel" not in name:
            continue
        taps = [a for a, op, _, _ in ins if is_tap(op)]
        around = [(a, t) for a, t in branch_edges(ins) if t <= taps[0] and a >= taps[-1]]
        head = max(t for _, t in around)
        end = max(a for a, t in around if t == head)
        res[kernel_title(name)] = sum(1 for a, op, text, _ in ins if not head <= a <= end and category(op, text) in VALU)
    return res


def main():
    if "--outside-valu" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--outside-valu"]
        lib = os.path.abspath(rest[0]) if rest else LIB
        print("static VALU outside the level loop, per thread, from %s" % os.path.relpath(lib, ROOT))
        for title, n in sorted(outside_valu(lib).items()):
            print("  %-55s %5d" % (title, n))
        return
    if "--state-copies" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--state-copies"]
        state_copies_report(os.path.abspath(rest[0]) if rest else LIB)
        return
    if "--window-loads" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--window-loads"]
        window_loads_report(os.path.abspath(rest[0]) if rest else LIB)
        return
    defines = [a for a in sys.argv[1:] if a.startswith("-D")]
    srcs = [a for a in sys.argv[1:] if not a.startswith("-")]         # another revision of the file (git show REV:... > /tmp/x.hip)
    bl = blocks(kernel_text(defines, srcs[0] if srcs else SRC))
    # the level loop: the depth-2 loop that holds barriers
    heads = collections.Counter()
    for lab, ann, ins in bl:
        m = re.search(r"Header=(BB\d+_\d+) Depth=2", ann)
        if m and any(op == "s_barrier" for op, _ in ins):
            heads[m.group(1)] += 1
    head = heads.most_common(1)[0][0]
    in_loop = [b for b in bl if re.search(r"(Header=%s Depth=2|Parent Loop %s)" % (head, head), b[1]) or b[0] == "." + head[0:0] + "L" + head]
    cases, common = {}, collections.Counter()
    seq = [(lab, count(ins), ins) for lab, ann, ins in in_loop]
    i = 0
    pend = []
    while i < len(seq):
        lab, c, ins = seq[i]
        muls = sum(1 for op, _ in ins if op.startswith("v_mul_f64"))
        if muls == 0:
            common.update(c)
            i += 1
            continue
        pend.append((lab, c, ins, muls))
        i += 1
    # case blocks come in layout order main, pieces, (barrier) axis-1: split the axis-1 block at its barrier
    k = 0
    while k < len(pend):
        lab, c, ins, muls = pend[k]
        r = muls // 8 - 1
        main_c = c
        pieces_c, h_c = collections.Counter(), collections.Counter()
        k += 1
        if k < len(pend) and pend[k][3] == 4 * (r + 1):
            pieces_c = pend[k][1]
            k += 1
        if k < len(pend) and pend[k][3] == 8 * (r + 1):
            h_c = pend[k][1]
            k += 1
        else:       # no separate pieces block found: the axis-1 pass may share a block -- report as is
            pass
        cases[r] = (main_c, pieces_c, h_c)
    radii = [4, 4, 4, 4, 5, 5, 5, 6, 6, 6, 7, 7, 8, 8, 9, 10, 10, 11, 12, 12, 13, 14]      # the 22 distinct blurs of octaves (1.6, 3.2)
    print("static census of one wave's level loop, fused kernel (default tile, band source)%s" % (("  [" + " ".join(defines) + "]") if defines else ""))
    print("blocks in the level loop: %d; radius cases found: %s" % (len(in_loop), sorted(cases)))
    print()
    print("per thread and level, common part (all radii): tap fetch, dispatch, DoG, edge strip, maxima, sieve, statistics, state moves")
    for cat in CATS:
        if common[cat]:
            print("  %-20s %5d" % (cat, common[cat]))
    print("  %-20s %5d" % ("VALU total", sum(common[c] for c in VALU)))
    # pure copies: per-pixel state renamed once per level (Dc = d, gprev = g: 2 K with one static register assignment) and
    # whatever else the compiler copies -- merged accumulators behind the radius switch, a second set of maxima
    print("  %-20s %5d   (v_mov_b64 from a VGPR pair, of the v_mov_b64 above; floor 16 = one rename each of D and G)"
          % ("state copies", sum(1 for lab, ann, ins in in_loop for op, text in ins if is_pair_copy(op, text))))
    print()
    # the blocks behind the level's second barrier (the last s_barrier of the loop in layout order): 3 x 3 maxima, sieve bits,
    # sieve, statistics, wave reduction, state renames.  A wave that owns a tested pixel runs, at a tested level (kl >= 4),
    # every one of them except the blocks that load constants into registers (zero maxima of an untested wave, the {inf, 0}
    # statistics of a wave or level without a sieve): wherever the compiler puts the renames, they are counted on that path.
    last = max(i for i, b in enumerate(in_loop) if any(op == "s_barrier" for op, _ in b[2]))
    tail = [(in_loop[last][0], in_loop[last][2][[op for op, _ in in_loop[last][2]].index("s_barrier") + 1:])] + \
           [(lab, ins) for lab, ann, ins in in_loop[last + 1:]]
    print("behind the second barrier, per thread and level: issue slots by block (one slot = one FP64 issue, 4 cycles; table in the script)")
    print("  block        VALU  slots  DPP  fp64 cmp  selects  folds  s_nop")
    tested, tested_valu = 0.0, 0
    for lab, ins in tail:
        c = count(ins)
        if not sum(c[x] for x in VALU) and not any(op == "s_nop" for op, _ in ins):
            continue
        on_path = not any(re.match(r"v_mov_b(64|32)\S*\s+v\S+,\s+(0|0x7ff00000)$", text) for _, text in ins)
        tested += slots(ins) if on_path else 0.0
        tested_valu += sum(c[x] for x in VALU) if on_path else 0
        print("  %-10s %5d  %5.1f  %3d  %8d  %7d  %5d  %5d%s" % (lab.lstrip("."), sum(c[x] for x in VALU), slots(ins), c["DPP move"], c["fp64 compare"],
                                                              c["v_cndmask"], sum(1 for op, text in ins if is_fold(op, text)),
                                                              sum(1 for op, _ in ins if op == "s_nop"), "   <- tested wave" if on_path else ""))
    print("  all blocks (static)                     %6.1f slots" % sum(slots(ins) for _, ins in tail))
    print("  tested wave at a tested level (marked blocks: maxima, sieve, statistics, renames)  %6.1f slots, %d VALU" % (tested, tested_valu))
    print()
    print("per thread and level, radius cases: axis-0 main | axis-0 leftover pieces (first 16 r threads) | axis-1")
    print("  r   blur flops (main, pieces, axis-1)   other VALU (main, pieces, axis-1)   LDS reads   LDS writes")
    tot_blur = tot_other = tot_common = 0.0
    for r in sorted(cases):
        m, p, h = cases[r]
        oth = lambda c: sum(c[x] for x in VALU) - c["fp64 add/mul"]
        print("  %2d  %5d %5d %5d                   %5d %5d %5d                  %4d %4d %4d   %4d %4d %4d"
              % (r, m["fp64 add/mul"], p["fp64 add/mul"], h["fp64 add/mul"], oth(m), oth(p), oth(h), m["LDS read"], p["LDS read"],
                 h["LDS read"], m["LDS write"], p["LDS write"], h["LDS write"]))
    print()
    # weighted per computed pixel: 256 threads per 30 x 62 owned pixels; pieces run on 16 r of the 256 threads
    px = 30 * 62
    for r in radii:
        if r not in cases:
            continue
        m, p, h = cases[r]
        share = min(1.0, 16.0 * r / 256.0)
        blur = m["fp64 add/mul"] + h["fp64 add/mul"] + share * p["fp64 add/mul"]
        other = sum((m[x] + h[x] + share * p[x]) for x in VALU) - blur
        tot_blur += blur
        tot_other += other
        tot_common += sum(common[x] for x in VALU)
    # the DoG's 8 subtractions sit in the common part and are fp64 add/mul there
    f = 256.0 / px
    print("per COMPUTED pixel over the 22 blurs of octaves (1.6, 3.2) (x 256 threads / %d owned pixels):" % px)
    print("  blur arithmetic (v_add/mul_f64 in the passes)        %7.1f" % (tot_blur * f))
    print("  other VALU inside the passes (addresses, moves)      %7.1f" % (tot_other * f))
    print("  common part VALU (DoG, maxima, sieve, stats, moves)  %7.1f   (all 22 levels counted with the full sieve: 18 run it, 4 only the maxima)"
          % (tot_common * f))
    print("  level loop total                                     %7.1f   (+ staging and epilogue outside the loop)"
          % ((tot_blur + tot_other + tot_common) * f))
    outside = collections.Counter()
    for lab, ann, ins in bl:
        if (lab, ann, ins) not in in_loop:
            outside.update(count(ins))
    print("  outside the loop, static VALU (staging loops run several times)  %d per thread = %.1f per pixel if run once"
          % (sum(outside[c] for c in VALU), sum(outside[c] for c in VALU) * f))
    src = srcs[0] if srcs else SRC
    located = kernel_text(list(defines) + ["-gline-tables-only"], src, keep_files=True)
    res = outside_by_path(located, src, {lab for lab, ann, ins in in_loop}, main_files(located, src))
    outside_report(res)
    # a second file names the revision of mst_diff.hip that goes with another revision of the fused kernel
    walk_report(src, defines, srcs[1] if len(srcs) > 1 else None if srcs else DIFF_SRC)


if __name__ == "__main__":
    main()
