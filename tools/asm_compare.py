#!/usr/bin/env python3
"""Compare two device assembly files function by function ("how to
check a pure refactor"): every function of `before` must be present in `after`
with the same body, and every .amdhsa_kernel with the same .amdhsa_* block.
Local labels carry the function's ordinal in the file (.LBB12_3), which moves
when functions are added ahead of it: the ordinal is dropped before comparing.

    hipcc <the Makefile's flags> --cuda-device-only -S -o before.s torj_hip.hip   (parent sources)
    hipcc <the Makefile's flags> --cuda-device-only -S -o after.s torj_hip.hip
    tools/asm_compare.py before.s after.s

Prints one line per function of either file and a summary; exit status 1 when a
function of `before` is missing or differs."""
import re
import subprocess
import sys

FUNC = re.compile(r"^\t\.type\t([^,\s]+),@function\s*$")
END = re.compile(r"^\.Lfunc_end\d+:")
KERN = re.compile(r"^\t?\.amdhsa_kernel\s+(\S+)")
LOCAL = re.compile(r"\.L(BB|tmp|func_begin|func_end|JTI|CPI)\d+(_\d+)?")


COMMENT_BB = re.compile(r"\bBB\d+_(\d+)")  # "in Loop: Header=BB12_3"


def norm(line):
    line = LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line.rstrip())
    return COMMENT_BB.sub(r"BB_\1", line)


def parse(path):
    # (a kernel's .amdhsa_kernel block lies between its last instruction and its .Lfunc_end label)
    bodies, blocks, cur, name, blk, kname = {}, {}, None, None, None, None
    with open(path) as f:
        for line in f:
            if blk is not None:
                if ".end_amdhsa_kernel" in line:
                    blocks[kname] = blk
                    blk = None
                else:
                    blk.append(norm(line))
                continue
            k = KERN.match(line)
            if k:
                kname, blk = k.group(1), []
                continue
            m = FUNC.match(line)
            if m:
                name, cur = m.group(1), []
            elif cur is not None:
                if END.match(line):
                    bodies[name] = cur
                    cur = None
                else:
                    cur.append(norm(line))
    return bodies, blocks


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(before, after):
    b_body, b_blk = parse(before)
    a_body, a_blk = parse(after)
    names = sorted(set(b_body) | set(a_body))
    pretty = demangle(names)
    bad = same = new = 0
    for n in names:
        kernel = n in b_blk or n in a_blk
        tag = "kernel  " if kernel else "function"
        if n not in a_body:
            state, bad = "MISSING in after", bad + 1
        elif n not in b_body:
            state, new = "new", new + 1
        elif b_body[n] != a_body[n]:
            state, bad = "BODY DIFFERS", bad + 1
        elif kernel and b_blk.get(n) != a_blk.get(n):
            state, bad = "AMDHSA BLOCK DIFFERS", bad + 1
        else:
            state, same = "identical" + (" (body and .amdhsa_* block)" if kernel else ""), same + 1
        print(f"{tag} {state:40s} {pretty[n]}")
    print(f"# {before} -> {after}: {same} identical, {new} new, {bad} missing or different")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
