#!/usr/bin/env python3
"""Static instruction counts of a merson_pair instance's z-loop for gfx950, per section between
two plane barriers.  Compiles pft_kernels.hip to assembly with the Makefile's flags (no GPU) and
counts instruction classes; nothing is timed.

    python scripts/pair_loop_isa.py [--src FILE] [--asm FILE] [INSTANCE ...] [-- extra hipcc flags]

INSTANCE: the template arguments "SA,MODE,GLX,LWP", e.g. 4,0,true,22 (default: 2,0,true,22 and
4,0,true,22, the kernels of the 400^3 benchmark).  --asm reads an assembly file made earlier instead
of compiling.  A section is the code between two s_barrier in layout order, tagged with the loop
depth the assembler's block comments give (a tree with the steady loop has it at depth 2 inside the
general loop's depth 1; one z-loop alone is depth 1).  Columns:

  instr   all instructions           fp64   v_*_f64 (rcp / rsq / div helpers included)
  valu    other v_* instructions     salu   s_* arithmetic, moves, compares, exec masks (no s_nop)
  nop     s_nop                      br     s_branch / s_cbranch_*
  sload   s_load_* (kernarg segment) wait   s_waitcnt
  iso     s_waitcnt lgkmcnt(0) whose last s_load lies at most two VALU instructions before it
  lds     ds_*                       vmem   global_* / buffer_* / flat_*
  lane    v_readlane / v_writelane (SGPR spill traffic)
  scr     scratch_* (VGPR spill traffic)
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-Wno-unused-result"]          # porousfreezethaw_amd/Makefile: HIPFLAGS
COLS = ["instr", "fp64", "valu", "salu", "nop", "br", "sload", "wait", "iso", "lds", "vmem", "lane", "scr"]


def classify(op):
    if op.startswith("s_load"):
        return "sload"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_nop":
        return "nop"
    if op.startswith("s_branch") or op.startswith("s_cbranch"):
        return "br"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_readlane") or op.startswith("v_writelane"):
        return "lane"
    if re.match(r"v_\w+_f64", op):
        return "fp64"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_"):
        return "scr"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    return "other"


def sections(lines):
    """[(first line number, loop depth, counts)] of the code between barriers"""
    out, cur, depth, start = [], dict.fromkeys(COLS, 0), 0, None
    since_load = None                     # VALU instructions since the last s_load

    def cut():
        nonlocal cur, start
        if cur["instr"]:
            out.append((start, depth, cur))
        cur, start = dict.fromkeys(COLS, 0), None

    for no, line in lines:
        text, _, comment = line.partition(";")
        text = text.strip()
        m = re.search(r"Depth=(\d+)", comment)
        new = None
        if text.endswith(":"):            # a block label: its loop from the assembler's comment
            if "Parent Loop" in comment:
                continue                  # an inner loop's header: its depth is on the next line
            new = int(m.group(1)) if m else 0
        elif not text and "=>" in comment and m:
            new = int(m.group(1))
        if new is not None and new != depth:
            cut()
            depth = new
        if not text or text.endswith(":") or text.startswith("."):
            continue
        op = text.split()[0]
        if start is None:
            start = no
        if op == "s_barrier":
            cur["instr"] += 1
            cut()
            since_load = None
            continue
        k = classify(op)
        cur["instr"] += 1
        if k in cur:
            cur[k] += 1
        if k == "sload":
            since_load = 0
        elif k in ("fp64", "valu") and since_load is not None:
            since_load += 1
        elif k == "wait" and "lgkmcnt(0)" in text:
            if since_load is not None and since_load <= 2:
                cur["iso"] += 1
            since_load = None
    cut()
    return out


def report(asm, inst):
    sa, mode, glx, lwp = [s.strip() for s in inst.split(",")]
    sym = f"_Z11merson_pairILi{sa}ELi{mode}ELb{1 if glx in ('true', '1') else 0}ELi{lwp}EEv8PairArgs10pft_consts"
    lines, on = [], False
    for no, line in enumerate(asm, 1):
        if line.startswith(sym + ":"):
            on = True
            continue
        if on and line.startswith(".Lfunc_end"):
            break
        if on:
            lines.append((no, line.rstrip("\n")))
    if not lines:
        print(f"merson_pair<{inst}>: not in the assembly")
        return
    secs = sections(lines)
    # the z-loop is the first loop of the kernel: the sections from its first to the next one
    # outside any loop (the epilogue's reduction loop comes after that)
    first = next((i for i, s in enumerate(secs) if s[1] > 0), len(secs))
    last = next((i for i in range(first, len(secs)) if secs[i][1] == 0), len(secs))
    secs = secs[first:last]
    print(f"merson_pair<{sa}, {mode}, {glx}, {lwp}>: {len(secs)} sections (cut at barriers and where the loop depth changes)")
    print("   sec   line depth " + " ".join(f"{c:>5s}" for c in COLS))
    for i, (start, depth, c) in enumerate(secs):
        if depth:
            print(f"  {i:4d} {start or 0:6d} {depth:5d} " + " ".join(f"{c[k]:5d}" for k in COLS))
    for d in sorted({s[1] for s in secs if s[1] > 0}):
        # a z-loop is unrolled into three plane steps
        body = [c for (_, dd, c) in secs if dd == d]
        print(f"  loop at depth {d}, per plane step (its sections' sum / 3): "
              + " ".join(f"{k} {sum(c[k] for c in body) / 3:.0f}" for k in COLS))


def main():
    args, extra = sys.argv[1:], []
    if "--" in args:
        i = args.index("--")
        args, extra = args[:i], args[i + 1:]
    src = os.path.join(REPO, "porousfreezethaw_amd", "csrc", "pft_kernels.hip")
    asm_file, insts = None, []
    while args:
        a = args.pop(0)
        if a == "--src":
            src = args.pop(0)
        elif a == "--asm":
            asm_file = args.pop(0)
        else:
            insts.append(a)
    insts = insts or ["2,0,true,22", "4,0,true,22"]
    if asm_file is None:
        tmp = tempfile.mkdtemp(prefix="pair_isa_")
        asm_file = os.path.join(tmp, "pft_kernels.s")
        hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
        cmd = [hipcc] + FLAGS + ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "porousfreezethaw_amd", "csrc"),
                                 "--cuda-device-only", "-S", src, "-o", asm_file] + extra
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    with open(asm_file) as f:
        asm = f.readlines()
    for inst in insts:
        report(asm, inst)
        print()


if __name__ == "__main__":
    main()
