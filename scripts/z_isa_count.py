#!/usr/bin/env python
"""Instruction counts of the z kernel's pair loop, from the compiler's assembly.  No GPU.

    python scripts/z_isa_count.py [--kernel true,false,2,7,false,false,true] [--asm FILE] [--keep FILE]

Compiles hmsc_amd/csrc/zdraw.hip for the device only with build.py's flags (FLAGS + EXTRA), or
reads --asm, and prints

  * for every z_wave_kernel instantiation: VGPRs, AGPRs, SGPRs, scratch bytes per lane, waves
    per SIMD and code bytes, and the sum of the code bytes;
  * for the instantiation --kernel names (its template arguments, in order): the blocks of the
    inner draw loop, `for (c = 0; c < 4; ++c)`, which of them are the hot path of one trip, and
    the hot path's instructions by class; the scratch and vmcnt instructions of the tile loop.

The hot path of a trip is what a wave issues when no lane leaves the table draw:
  - a region skipped by an exec-mask branch (s_cbranch_execz) is a tail -- the deep tail
    (alpha > 25) or AS241's -- if its own instructions, those outside the tails nested in it,
    hold a division or a square root (v_rcp / v_rsq / v_sqrt / v_div_*_f64); the table draw holds
    none.  A region that nests tails and holds no fp64 arithmetic of its own is the dispatch
    around them (which cell goes to which tail) and a tail too.  The exec-mask branches
    themselves are counted as not taken;
  - a block holding the marker comment `z_edge_trip` (z_kernel.h) and what is reached only
    through it is the guarded epilogue of a ragged wave tile, chosen by a uniform branch;
  - the Philox block (the one with the v_mad_u64_u32 rounds) is issued on every second trip and
    counts half.
Classes: fp64 arithmetic = v_fma / v_fmac / v_mul / v_add_f64; Philox = v_mad_u64_u32 and
v_bitop3_b32 of the Philox block; other VALU = every other v_ instruction; SALU = s_ except
s_waitcnt / s_nop (listed as waits); LDS = ds_; VMEM = global_ / flat_ / buffer_ / scratch_.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOW = re.compile(r"^v_(rcp|rsq|sqrt|div_fmas|div_fixup|div_scale)_f64")
FP64 = re.compile(r"^v_(fma|fmac|mul|add)_f64")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BBCOM = re.compile(r"^; %(bb\.\d+):")
BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)")
EDGE_MARK = "z_edge_trip"


def compile_asm(out):
    from hmsc_amd import build as B
    src = os.path.join(B.CSRC, "zdraw.hip")
    cmd = [B.HIPCC] + B.FLAGS + B.EXTRA.get("zdraw.hip", []) + ["-x", "hip", "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def mangled_args(spec):
    out = ""
    for tok in spec.replace(" ", "").split(","):
        out += {"true": "Lb1E", "false": "Lb0E"}.get(tok) or ("Li%dE" % int(tok))
    return "z_wave_kernelI" + out + "EEv"


def demangle_args(name):
    m = re.search(r"z_wave_kernelI((?:L[bi]\d+E)+)E", name)
    toks = re.findall(r"L([bi])(\d+)E", m.group(1))
    return ", ".join(("true" if v == "1" else "false") if k == "b" else v for k, v in toks)


def functions(lines):
    """name -> (first line, last line) of every z_wave_kernel, and its resource comments."""
    fns, cur, start = OrderedDict(), None, 0
    for n, ln in enumerate(lines):
        m = re.match(r"^(_ZN4hmsc13z_wave_kernelI\w+):", ln)
        if m:
            cur, start = m.group(1), n
        elif cur and ln.startswith(".Lfunc_end"):
            fns[cur] = dict(lo=start, hi=n)
            info = {}
            for ln2 in lines[n:n + 60]:
                m2 = re.match(r"^; (codeLenInByte|TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy)\s*[:=]\s*(\d+)", ln2)
                if m2:
                    info[m2.group(1)] = int(m2.group(2))
            fns[cur].update(info)
            cur = None
    return fns


class Block:
    def __init__(self, name, header, depth):
        self.name, self.header, self.depth = name, header, depth
        self.ins, self.marks = [], False

    def targets(self):
        return [(m.group(1), m.group(2)) for m in (BRANCH.match(i) for i in self.ins) if m]

    def falls_through(self):
        return not self.ins or not re.match(r"^(s_branch|s_endpgm|s_setpc)", self.ins[-1])


def blocks_of(lines):
    """The function's basic blocks in layout order; loop membership from the compiler's comments."""
    out, cur = [], Block("entry", None, 0)
    out.append(cur)
    for n, ln in enumerate(lines):
        s = ln.strip()
        m = LABEL.match(ln) or BBCOM.match(ln)
        if m:
            com = ln  # the label's comment and its continuation lines
            for ln2 in lines[n + 1:n + 8]:
                if not re.match(r"^\s+;", ln2):
                    break
                com += ln2
            h = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", com)
            d = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", com)
            if h:
                header, depth = ".L" + h.group(1), int(h.group(2))
            elif d:
                header, depth = m.group(1), int(d.group(1))
            else:
                header, depth = None, 0
            cur = Block(m.group(1), header, depth)
            out.append(cur)
            continue
        if EDGE_MARK in s:
            cur.marks = True
        if not s or s.startswith(";") or s.startswith("."):
            continue
        cur.ins.append(s.split(";")[0].strip())
    return out


def classify(b, philox):
    c = dict(fp64=0, philox=0, valu=0, salu=0, wait=0, lds=0, vmem=0)
    for i in b.ins:
        op = i.split()[0]
        if FP64.match(op):
            c["fp64"] += 1
        elif philox and (op.startswith("v_mad_u64_u32") or op.startswith("v_bitop3_b32")):
            c["philox"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op in ("s_waitcnt", "s_nop"):
            c["wait"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif re.match(r"^(global|flat|buffer|scratch)_", op):
            c["vmem"] += 1
    return c


def analyse(lines, label):
    blks = blocks_of(lines)
    # the draw loop: the depth-2 loop holding the Philox rounds
    hdr = None
    for b in blks:
        if b.depth == 2 and sum(i.startswith("v_mad_u64_u32") for i in b.ins) >= 10:
            hdr = b.header
    if hdr is None:
        print(f"{label}: no inner loop with Philox rounds (not a drawing probit kernel)")
        return
    loop = [b for b in blks if b.header == hdr]
    idx = {b.name: k for k, b in enumerate(loop)}
    # tails: regions skipped by an exec-mask branch whose own instructions hold a division / sqrt
    regions = []
    for k, b in enumerate(loop):
        for op, t in b.targets():
            if op == "s_cbranch_execz" and t in idx and idx[t] > k + 1:
                regions.append((k + 1, idx[t]))
    cold = set()
    for lo, hi in sorted(regions, key=lambda r: r[1] - r[0]):
        own = [loop[k] for k in range(lo, hi) if k not in cold]
        nested = any(k in cold for k in range(lo, hi))
        slow = any(SLOW.match(i.split()[0]) for b in own for i in b.ins)
        glue = nested and not any(FP64.match(i.split()[0]) for b in own for i in b.ins)
        if slow or glue:
            cold |= set(range(lo, hi))
    # the hot path: reachable from the header without passing a tail or a marked block
    hot, todo = set(), [idx[hdr]]
    while todo:
        k = todo.pop()
        if k in hot or k in cold or loop[k].marks:
            continue
        hot.add(k)
        b = loop[k]
        for _, t in b.targets():
            if t in idx and t != hdr:
                todo.append(idx[t])
        if b.falls_through() and k + 1 < len(loop):
            todo.append(k + 1)
    tot = dict(fp64=0.0, philox=0.0, valu=0.0, salu=0.0, wait=0.0, lds=0.0, vmem=0.0)
    print(f"draw loop of {label}: header {hdr}, {len(loop)} blocks")
    print("  block        path      fp64 philox  valu  salu  wait   lds  vmem")
    for k, b in enumerate(loop):
        philox = sum(i.startswith("v_mad_u64_u32") for i in b.ins) >= 10
        c = classify(b, philox)
        kind = "tail" if k in cold else ("edge" if k not in hot else ("hot/2" if philox else "hot"))
        if not b.ins:
            continue
        print(f"  {b.name:<12} {kind:<8} {c['fp64']:>5} {c['philox']:>6} {c['valu']:>5} {c['salu']:>5} {c['wait']:>5} "
              f"{c['lds']:>5} {c['vmem']:>5}")
        if k in hot:
            for key in tot:
                tot[key] += c[key] * (0.5 if philox else 1.0)
    print("hot path of one trip (the Philox block at half weight):")
    print(f"  fp64 arithmetic {tot['fp64']:g} | Philox mul / bitop {tot['philox']:g} | other VALU {tot['valu']:g} | "
          f"all VALU {tot['fp64'] + tot['philox'] + tot['valu']:g}")
    print(f"  SALU {tot['salu']:g} | s_waitcnt / s_nop {tot['wait']:g} | LDS {tot['lds']:g} | VMEM {tot['vmem']:g}")
    # the tile loop around it: scratch traffic and the vmcnt waits, in program order
    lo = min(k for k, b in enumerate(blks) if b.header == hdr)
    tile_hdr = None
    for b in reversed(blks[:lo]):
        if b.depth == 1 and b.header:
            tile_hdr = b.header
            break
    tile = [b for b in blks if b.header in (tile_hdr, hdr)]
    nscr = sum(i.startswith("scratch_") for b in tile for i in b.ins)
    print(f"tile loop {tile_hdr}: {nscr} scratch instructions inside it")
    print("  vmcnt waits and VMEM of the tile loop in program order (runs folded):")
    run, last = 0, None
    for b in tile:
        where = "draw" if b.header == hdr else "tile"
        if b.header == hdr:
            k = idx[b.name]
            where = "draw " + ("tail" if k in cold else "edge" if k not in hot else "hot")
        for i in b.ins:
            op = i.split()[0]
            key = None
            if op == "s_waitcnt" and "vmcnt" in i:
                key = f"{where:<10} {b.name:<12} {i}"
            elif re.match(r"^(global|flat|buffer|scratch)_", op):
                key = f"{where:<10} {b.name:<12} {op}"
            if key is None:
                continue
            if key == last:
                run += 1
                continue
            if last is not None:
                print("    " + last + (f" x{run}" if run > 1 else ""))
            last, run = key, 1
    if last is not None:
        print("    " + last + (f" x{run}" if run > 1 else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="true,false,2,7,false,false,true",
                    help="template arguments of the instantiation whose draw loop is counted")
    ap.add_argument("--asm", default=None, help="read this assembly instead of compiling")
    ap.add_argument("--keep", default=None, help="write the compiled assembly here")
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = args.keep or os.path.join(tempfile.mkdtemp(prefix="zisa_"), "zdraw.s")
        compile_asm(path)
    with open(path) as f:
        lines = f.read().split("\n")
    fns = functions(lines)
    from hmsc_amd import build as B
    print("hipcc " + " ".join(B.FLAGS + B.EXTRA.get("zdraw.hip", [])) + " -x hip --cuda-device-only -S hmsc_amd/csrc/zdraw.hip")
    print("z_wave_kernel<DRAW, HAS_NA, NKB, MODE, POIS, NORMAL[, LEAN]> | VGPR AGPR SGPR scratch waves/SIMD code bytes")
    total = 0
    for name, f in fns.items():
        total += f.get("codeLenInByte", 0)
        print(f"<{demangle_args(name)}> | V{f.get('NumVgprs')} A{f.get('NumAgprs')} S{f.get('TotalNumSgprs')} "
              f"scr{f.get('ScratchSize')} occ{f.get('Occupancy')} {f.get('codeLenInByte')}")
    print(f"{len(fns)} instantiations, {total} code bytes; the assembly is {len(lines)} lines")
    want = mangled_args(args.kernel)
    hit = [n for n in fns if want in n]
    if not hit:
        sys.exit(f"no instantiation z_wave_kernel<{args.kernel}> in the assembly")
    f = fns[hit[0]]
    analyse(lines[f["lo"]:f["hi"]], f"z_wave_kernel<{args.kernel}>")


if __name__ == "__main__":
    main()
