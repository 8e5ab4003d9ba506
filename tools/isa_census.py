#!/usr/bin/env python3
"""Static census of the instructions of device kernels, per loop.

  python tools/isa_census.py KERNEL [KERNEL ...] [--define NAME ...] [--asm FILE] [--top N]

Compiles blu_amd/csrc/blu_hip.hip to gfx950 assembly with the flags of blu_amd/csrc/Makefile into a temporary directory
(or reads --asm FILE, an assembly file made before) and prints, for every kernel named and for every loop the compiler
labels in it (header block, depth, parent loop), how many instructions of each class the loop holds:

  valu       v_* instructions                      salu    s_* instructions that are not loads
  sload      s_load_* / s_buffer_load_*            reload  v_readlane_b32 into an SGPR from a VGPR marked as SGPR spill lanes
  spillwr    v_writelane_b32 into such a VGPR      vmov    v_mov_* / v_accvgpr_*
  snop       s_nop                                 scr_ld / scr_st   scratch_load_* / scratch_store_*
  flat       flat_*                                g_sbase / g_vaddr global_* with a scalar base / with a 64-bit vector address
  lds        ds_*                                  addr64  v_lshl_add_u64, v_lshlrev_b64, v_add_co / v_addc pairs count once (v_addc)
  sext       v_ashrrev_i32 v, 31, v

"self" rows count the blocks whose innermost loop is that loop, "incl" rows add the loops nested in it; a loop is listed
from --top instructions of its own (default 150), and all loops of one depth are summed at the end.  Then the spill
lanes: per (VGPR, lane) the number of reloads in the kernel and in each loop depth, and the blocks that write the lane.
Last the resource lines of the kernel (registers, scratch, LDS, occupancy).  The tool counts instructions by class; it
looks for nothing else.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blu_amd", "csrc")

CLASSES = ["valu", "salu", "sload", "reload", "spillwr", "vmov", "snop", "scr_ld", "scr_st", "flat", "g_sbase", "g_vaddr",
           "lds", "addr64", "sext", "other"]


def makefile_var(name):
    with open(os.path.join(CSRC, "Makefile")) as f:
        for line in f:
            m = re.match(r"%s\s*\??:?=\s*(.*)" % re.escape(name), line)
            if m:
                return m.group(1).strip()
    raise SystemExit("no %s in the Makefile" % name)


def compile_asm(defines, tmp):
    hipcc = os.environ.get("HIPCC", makefile_var("HIPCC"))
    arch = os.environ.get("ARCH", makefile_var("ARCH"))
    out = os.path.join(tmp, "blu_hip.s")
    cmd = [hipcc, "--offload-arch=" + arch] + makefile_var("FLAGS").split() + ["-D" + d for d in defines] + \
          ["--offload-device-only", "-S", "blu_hip.hip", "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True)
    return out


def split_functions(lines):
    """name -> (first line, line of .Lfunc_end) of every function of the file"""
    funcs = {}
    cur = None
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_][\w.$]*):", l)
        if m and not l.startswith(".L"):
            cur = (m.group(1), i)
        elif l.startswith(".Lfunc_end") and cur:
            funcs[cur[0]] = (cur[1], i)
            cur = None
    return funcs


def find_kernel(funcs, name):
    key = "%d%sE" % (len(name), name)  # the Itanium mangling of the last name component
    hits = [f for f in funcs if key in f or f == name]
    if len(hits) != 1:
        raise SystemExit("kernel %s: %d functions match (%s)" % (name, len(hits), ", ".join(hits[:5])))
    return hits[0]


def classify(mn, ops, spill_vgprs):
    if mn == "v_readlane_b32":
        p = [o.strip() for o in ops.split(",")]
        if len(p) == 3 and p[0].startswith("s") and p[1] in spill_vgprs:
            return "reload", (p[1], p[2])
        return "valu", None
    if mn == "v_writelane_b32":
        p = [o.strip() for o in ops.split(",")]
        if len(p) == 3 and p[0] in spill_vgprs:
            return "spillwr", (p[0], p[2], p[1])
        return "valu", None
    if mn.startswith("v_mov_") or mn.startswith("v_accvgpr_"):
        return "vmov", None
    if mn.startswith(("v_lshl_add_u64", "v_lshlrev_b64", "v_addc_co")):
        return "addr64", None
    if mn.startswith("v_ashrrev_i32") and re.match(r"\s*v\d+\s*,\s*31\s*,\s*v\d+", ops):
        return "sext", None
    if mn.startswith("v_"):
        return "valu", None
    if mn == "s_nop":
        return "snop", None
    if mn.startswith("s_load_") or mn.startswith("s_buffer_load_"):
        return "sload", None
    if mn.startswith("s_"):
        return "salu", None
    if mn.startswith("scratch_load"):
        return "scr_ld", None
    if mn.startswith("scratch_"):
        return "scr_st", None
    if mn.startswith("flat_"):
        return "flat", None
    if mn.startswith("global_"):
        # global_load  vdst, vaddr, saddr|off     global_store vaddr, vdata, saddr|off     (atomics: like stores, rtn first)
        p = [o.strip() for o in ops.split(",")]
        last = p[-1].split()[0] if p else ""
        return ("g_sbase" if last.startswith("s[") else "g_vaddr"), None
    if mn.startswith("ds_"):
        return "lds", None
    return "other", None


VECTOR = ("valu", "reload", "spillwr", "vmov", "addr64", "sext")  # what goes through the vector ALU


def census(lines, name, first, last, top):
    body = lines[first:last]
    spill_vgprs = set()
    for l in body:
        m = re.search(r"implicit-def: \$(vgpr\d+)\s*:\s*SGPR spill to VGPR lane", l)
        if m:
            spill_vgprs.add("v" + m.group(1)[4:])
    # blocks and their loops
    loops = {}  # header -> (depth, parent header or None)
    cur_loop, cur_block = None, "entry"
    per = collections.defaultdict(collections.Counter)  # loop header (None = outside) -> class -> n
    reload_by_lane = collections.defaultdict(collections.Counter)  # (vgpr, lane) -> depth -> n
    writes = collections.defaultdict(list)
    i = 0
    n = len(body)
    while i < n:
        l = body[i]
        mlab = re.match(r"^(\.LBB\d+_\d+):", l)
        mbb = re.match(r"^; %bb\.(\d+):", l)
        if mlab or mbb:
            cur_block = mlab.group(1)[2:] if mlab else "bb." + mbb.group(1)
            # the comments of the block: the rest of this line and the comment-only lines that follow
            notes = [l]
            j = i + 1
            while j < n and re.match(r"^\s+;", body[j]):
                notes.append(body[j])
                j += 1
            text = "\n".join(notes)
            parents = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", text)
            mh = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", text)
            mi = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", text)
            if mh:
                depth = int(mh.group(1))
                parent = None
                for p, d in parents:
                    if int(d) == depth - 1:
                        parent = p
                loops[cur_block] = (depth, parent)
                cur_loop = cur_block
            elif mi:
                cur_loop = mi.group(1)
                if cur_loop not in loops:
                    loops[cur_loop] = (int(mi.group(2)), None)
            else:
                cur_loop = None
            i = j
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)\s*(.*?)\s*(?:;.*)?$", l)
        if m and not l.lstrip().startswith("."):
            mn, ops = m.group(1), m.group(2)
            cls, info = classify(mn, ops, spill_vgprs)
            per[cur_loop][cls] += 1
            depth = loops[cur_loop][0] if cur_loop else 0
            if cls == "reload":
                reload_by_lane[info][depth] += 1
            elif cls == "spillwr":
                writes[(info[0], info[1])].append("%s(d%d)<-%s" % (cur_block, depth, info[2]))
        i += 1

    def incl(h):
        c = collections.Counter(per[h])
        for k, (d, p) in loops.items():
            if p == h:
                c.update(incl(k))
        return c

    print("=" * 120)
    print("kernel %s" % name)
    print("spill-lane VGPRs: %s" % (", ".join(sorted(spill_vgprs, key=lambda v: int(v[1:]))) or "none"))
    hdr = "%-22s %-5s %-10s %6s " % ("loop", "depth", "parent", "vector") + " ".join("%7s" % c for c in CLASSES)

    def row(tag, d, p, c):
        vec = sum(c[k] for k in VECTOR)
        print("%-22s %-5s %-10s %6d " % (tag, d, p or "-", vec) + " ".join("%7d" % c[k] for k in CLASSES))

    print(hdr)
    total = collections.Counter()
    for c in per.values():
        total.update(c)
    row("whole kernel", "-", None, total)
    row("outside loops", "0", None, per[None])
    by_depth = collections.defaultdict(collections.Counter)
    for h in sorted(loops, key=lambda k: [int(x) for x in re.findall(r"\d+", k)]):
        d, p = loops[h]
        by_depth[d].update(per[h])
        if sum(per[h].values()) >= top:
            row(h + " self", d, p, per[h])
            if any(pp == h for (_, pp) in loops.values()):
                row(h + " incl", d, p, incl(h))
    print("-- all loops of one depth together (self counts)")
    for d in sorted(by_depth):
        row("depth %d" % d, d, None, by_depth[d])
    print("-- reloads of spilled scalars per (VGPR, lane): total, per loop depth; blocks that write the lane")
    depths = sorted({d for c in reload_by_lane.values() for d in c})
    print("%-6s %-5s %6s " % ("vgpr", "lane", "total") + " ".join("%5s" % ("d%d" % d) for d in depths) + "  written in")
    for (v, ln), c in sorted(reload_by_lane.items(), key=lambda kv: -sum(kv[1].values())):
        w = writes.get((v, ln), [])
        print("%-6s %-5s %6d " % (v, ln, sum(c.values())) + " ".join("%5d" % c[d] for d in depths) + "  " +
              (" ".join(w[:4]) + (" ..." if len(w) > 4 else "")))
    print("-- resources")
    for l in lines[last:last + 120]:
        m = re.match(r"^;\s*(NumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize|SGPRBlocks|VGPRBlocks|"
                     r"codeLenInByte|MemoryBound)\s*:.*", l)
        if m:
            print("  " + l[1:].strip())
        if l.startswith(".Lfunc_begin") or re.match(r"^\s+\.type\s", l):
            break


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernels", nargs="+")
    ap.add_argument("--define", action="append", default=[], help="extra -D of the build (BLU_PROFILE, ...)")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    ap.add_argument("--top", type=int, default=150, help="list a loop only from this many instructions of its own")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = a.asm or compile_asm(a.define, tmp)
        with open(path) as f:
            lines = f.read().split("\n")
    funcs = split_functions(lines)
    for k in a.kernels:
        f = find_kernel(funcs, k)
        census(lines, f, funcs[f][0], funcs[f][1], a.top)
    return 0


if __name__ == "__main__":
    sys.exit(main())
