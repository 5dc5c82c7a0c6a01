#!/usr/bin/env python3
"""Instruction census of the cell-tiled trajectory kernel's stage loop.

Compiles torj.jl_amd/csrc/torj_traj.hip to gfx950 assembly with the Makefile's
HIPFLAGS and TRAJ_FLAGS (device only, -S) and prints, for every basic block of
the stage loop of one k_traj_cell instance (the depth-2 loop with the most
instructions: cold_step's `for st`), how many instructions of each class it
holds -- classified by mnemonic alone:

  fp64   VALU fp64 arithmetic (add, mul, fma, fmac, max, min, rcp, rsq, ldexp,
         floor, rndne ... on f64 operands)
  valu   every other VALU instruction (moves, selects, compares, conversions,
         integer and address arithmetic)
  salu   scalar ALU and control (s_*, without s_waitcnt / s_nop)
  lds    ds_*
  glob   global_* / flat_* / buffer_* / scratch_*
  wait   s_waitcnt, s_nop

then the loop's totals, the most frequent `valu` mnemonics (where the non-fp64
work sits) and the kernel's register / scratch footer.  A block is on the hot
path or not by the branch structure, which the census does not judge: read the
blocks' sizes (the two large lds-only blocks are the in-tile evaluations of
stage 0, with psi, and of stages 1-3).

usage: python tools/traj_isa_census.py [-DFLAG=V ...] [--kernel MANGLED_SUBSTRING]
                                       [--asm FILE] [--keep FILE] [--path BLOCK,BLOCK,...]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torj.jl_amd", "csrc")

FP64_OPS = ("add", "mul", "fma", "fmac", "max", "min", "rcp", "rsq", "sqrt", "ldexp", "floor", "ceil", "trunc",
            "rndne", "fract", "div_scale", "div_fmas", "div_fixup", "frexp_mant")
FP64_RE = re.compile(r"^v_(?:%s)_f64(?:_e32|_e64|_dpp|_sdwa)?$" % "|".join(FP64_OPS))
CLASSES = ("fp64", "valu", "salu", "lds", "glob", "wait")


def classify(mn):
    if mn in ("s_waitcnt", "s_nop") or mn.startswith("s_waitcnt"):
        return "wait"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "glob"
    if mn.startswith("v_"):
        return "fp64" if FP64_RE.match(mn) else "valu"
    return None


def make_var(name):
    """the default a `NAME ?= value` line of the Makefile gives"""
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"^%s\s*\?=\s*(.*)$" % re.escape(name), line)
        if m:
            return m.group(1).split()
    raise SystemExit("csrc/Makefile has no %s ?=" % name)


def compile_asm(defs, out):
    hipcc = os.environ.get("HIPCC", make_var("HIPCC")[0])
    cmd = [hipcc] + make_var("HIPFLAGS") + defs + make_var("TRAJ_FLAGS") + ["--cuda-device-only", "-S", "-o", out,
                                                                          "torj_traj.hip"]
    r = subprocess.run(cmd, cwd=CSRC, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit("compile failed: " + " ".join(cmd))
    return " ".join(make_var("HIPFLAGS") + defs + make_var("TRAJ_FLAGS"))


def kernel_body(lines, key):
    label = re.compile(r"^(_Z\S*):") if not key else re.compile(r"^(\S*%s\S*):" % re.escape(key))
    start = next((k for k, l in enumerate(lines) if label.match(l)), None)
    if start is None:
        raise SystemExit("no kernel matching %r" % key)
    end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
    return label.match(lines[start]).group(1), lines[start + 1:end], lines[end:]


def blocks_of(body):
    """[[name, loop header, loop depth, [mnemonics]]] in layout order (depth 0: in no loop)"""
    out = [["entry", None, 0, []]]
    for raw in body:
        line = raw.strip()
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):\s*(?:;(.*))?$", line)
        if m:
            name, note = m.group(1).lstrip("; "), m.group(2) or ""
            self_hdr = name[2:] if name.startswith(".L") else name
            cur = [name, None, 0, []]
            hd = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", note)
            own = re.search(r"Loop Header: Depth=(\d+)", note)
            if hd:
                cur[1:3] = [hd.group(1), int(hd.group(2))]
            elif own:
                cur[1:3] = [self_hdr, int(own.group(1))]
            elif "Parent Loop" in note:
                cur[1] = self_hdr  # a nested loop's header: its depth is on a line below
            out.append(cur)
            continue
        m = re.match(r"^;\s*=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", line)
        if m and out[-1][1] and not out[-1][3]:
            out[-1][2] = int(m.group(1))
            continue
        if not line or line.startswith((";", ".", "//")):
            continue
        mn = line.split()[0]
        if classify(mn):
            out[-1][3].append(mn)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", default="k_traj_cellILi2ELb1EE", help="substring of the mangled kernel name")
    ap.add_argument("--asm", help="an assembly file to read instead of compiling")
    ap.add_argument("--keep", help="write the compiled assembly here")
    ap.add_argument("--label", default="", help="a title for the report")
    ap.add_argument("--path", default="", help="comma-separated blocks (as printed, e.g. .LBB0_65,%%bb.81) to sum "
                                               "as one path through the loop -- the reader's choice of path")
    args, defs = ap.parse_known_args()
    bad = [d for d in defs if not d.startswith("-D")]
    if bad:
        ap.error("unknown arguments: %s" % " ".join(bad))
    if args.asm:
        flags, path = "(read from %s)" % os.path.basename(args.asm), args.asm
    else:
        path = args.keep or os.path.join(tempfile.mkdtemp(prefix="traj_census_"), "torj_traj.s")
        flags = compile_asm(defs, path)
    lines = open(path).read().splitlines()
    name, body, rest = kernel_body(lines, args.kernel)
    blocks = blocks_of(body)
    # the stage loop: the depth-2 loop with the most instructions
    size = collections.Counter()
    for _, hdr, depth, ins in blocks:
        if depth == 2:
            size[hdr] += len(ins)
    if not size:
        raise SystemExit("no depth-2 loop in %s" % name)
    loop = size.most_common(1)[0][0]
    print("# traj_isa_census %s" % args.label)
    print("# flags: %s" % flags)
    print("# kernel: %s" % name)
    print("# stage loop: header %s" % loop)
    print("%-12s" % "block" + "".join("%7s" % c for c in CLASSES))
    tot = collections.Counter()
    other = collections.Counter()
    want = [b for b in args.path.split(",") if b]
    path = collections.Counter()
    seen = set()
    for bname, hdr, depth, ins in blocks:
        if depth != 2 or hdr != loop:
            continue
        c = collections.Counter(classify(m) for m in ins)
        tot.update(c)
        if bname in want:
            path.update(c)
            seen.add(bname)
        other.update(re.sub(r"_e(32|64)$", "", m) for m in ins if classify(m) == "valu")
        print("%-12s" % bname + "".join("%7d" % c[k] for k in CLASSES))
    print("%-12s" % "loop total" + "".join("%7d" % tot[k] for k in CLASSES))
    if want:
        if seen != set(want):
            raise SystemExit("--path: not in the loop: %s" % sorted(set(want) - seen))
        print("%-12s" % "path total" + "".join("%7d" % path[k] for k in CLASSES))
        print("# path: " + " ".join(want))
    print("# valu by mnemonic: " + ", ".join("%s %d" % kv for kv in other.most_common(14)))
    foot = [l.strip() for l in rest[:60] if re.match(r"^; (NumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize)", l)]
    print("# footer: " + "  ".join(f.lstrip("; ") for f in foot))


if __name__ == "__main__":
    main()
