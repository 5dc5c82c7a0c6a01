"""The head of an alpha wave and the register budgets beside it (DESIGN.md 3.7,
round 13), read from gfx950 assembly (no GPU needed).

k_alpha_pts<false>, compiled with csrc/Makefile's HIPFLAGS from
tests/native/alpha_isa.hip (the kernel alone behind the library's headers):
no scratch; at most 77 VGPRs, the parent commit's figure from the same compile
of its sources (commit df21cdf: NumVgprs 77, Occupancy 6); a wave of a flagged
group reaches s_endpgm on scalar instructions alone -- the group's word is a
scalar load, and nothing before its branch touches vector memory; a wave that
evaluates has issued ti, si and its five inputs before its one and only
s_waitcnt vmcnt ahead of the first fp64 instruction (the parent had two: the
flag byte's, then the inputs').

k_traj_cell, every instance, compiled as csrc/Makefile compiles torj_traj.hip,
now that it writes the group's word: at most 176 VGPRs, no scratch, and two
waves per SIMD or more (the headline's instance <2, true> exactly two:
tests/test_traj_resources.py)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = "_Z11k_alpha_ptsILb0EEv9TraceArgs9SplitArgsi"
PARENT_ALPHA_VGPRS = 77
VMEM = ("global_", "buffer_", "flat_", "scratch_")


def _census():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import traj_isa_census as census
    finally:
        sys.path.pop(0)
    return census


def _footer(rest):
    foot = {}
    for line in rest[:60]:
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", line)
        if m and m.group(1) not in foot:
            foot[m.group(1)] = int(m.group(2))
    return foot


@pytest.fixture(scope="module")
def alpha(tmp_path_factory):
    """(instructions of k_alpha_pts<false> in layout order, labels included; footer)"""
    census = _census()
    asm = str(tmp_path_factory.mktemp("alpha") / "alpha_isa.s")
    hipcc = os.environ.get("HIPCC", census.make_var("HIPCC")[0])
    subprocess.check_call([hipcc] + census.make_var("HIPFLAGS") +
                          ["-I" + census.CSRC, "--cuda-device-only", "-S", "-o", asm,
                           os.path.join(ROOT, "tests", "native", "alpha_isa.hip")])
    name, body, rest = census.kernel_body(open(asm).read().splitlines(), ALPHA)
    assert name == ALPHA
    ins = [l.split(";")[0].strip() for l in body]
    return [l for l in ins if l and not l.startswith((".p2align", ".cfi", ".loc", ".file"))], _footer(rest)


def test_alpha_registers(alpha):
    _, foot = alpha
    print(foot)
    assert foot["ScratchSize"] == 0, foot
    assert foot["NumVgprs"] <= PARENT_ALPHA_VGPRS, foot
    assert foot["Occupancy"] >= 6, foot


def _block(ins, label):
    """the instructions of the block `label` up to the next label"""
    k = ins.index(label + ":")
    out = []
    for l in ins[k + 1:]:
        if l.endswith(":") or l.startswith("."):  # the next label, or the directives behind the code
            break
        out.append(l)
    return out


def test_flagged_wave_ends_without_vector_memory(alpha):
    ins, _ = alpha
    first_vmem = next(k for k, l in enumerate(ins) if l.startswith(VMEM))
    head = ins[:first_vmem]
    # the kernel arguments come from s[0:1]; the one scalar load from another base is the group's word
    word = [k for k, l in enumerate(head) if re.match(r"^s_load_dword\s+s\d+,\s*s\[(?!0:1\])", l)]
    assert len(word) == 1, head
    # ... waited for, tested, and branched on before any vector memory instruction: the first
    # conditional branch behind it leads the flagged wave to a block that only ends the program
    after = head[word[0] + 1:]
    assert any(l.startswith("s_waitcnt") and "lgkmcnt(0)" in l for l in after), after
    br = next(l for l in after if l.startswith("s_cbranch_"))
    target = br.split()[-1]
    assert _block(ins, target) == ["s_endpgm"], (br, _block(ins, target))
    # and the arguments the head needs were loaded in one batch: every scalar load from
    # s[0:1] ahead of the first fp64 instruction stands before the kernel's first s_waitcnt
    first_wait = next(k for k, l in enumerate(ins) if l.startswith("s_waitcnt"))
    first_f64 = next(k for k, l in enumerate(ins) if re.match(r"^v_\w+_f64", l))
    kernarg = [k for k, l in enumerate(ins[:first_f64]) if re.match(r"^s_load_\w+\s+\S+\s*s\[0:1\]", l)]
    assert kernarg and max(kernarg) < first_wait, [ins[k] for k in kernarg]


def test_evaluating_wave_waits_once(alpha):
    ins, _ = alpha
    first_f64 = next(k for k, l in enumerate(ins) if re.match(r"^v_\w+_f64", l))
    head = ins[:first_f64]
    waits = [k for k, l in enumerate(head) if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert len(waits) == 1, [head[k] for k in waits]
    # ti, si and the five inputs (and, without group words, the flag byte) are in flight by then
    loads = [l.split()[0] for l in head[:waits[0]] if l.startswith("global_load")]
    assert loads.count("global_load_dword") == 2 and loads.count("global_load_dwordx2") == 5, loads
    assert [l for l in head[waits[0]:] if l.startswith(VMEM)] == []


def test_k_traj_cell_budget(tmp_path):
    census = _census()
    asm = str(tmp_path / "torj_traj.s")
    census.compile_asm([], asm)
    lines = open(asm).read().splitlines()
    seen = 0
    for depo in (0, 1, 2):
        for traj in (0, 1):
            key = "_Z11k_traj_cellILi%dELb%dEEv9TraceArgs9SplitArgs" % (depo, traj)
            name, body, rest = census.kernel_body(lines, key)
            foot = _footer(rest)
            print(name, foot)
            assert name == key
            assert foot["NumVgprs"] <= 176 and foot["ScratchSize"] == 0 and foot["Occupancy"] >= 2, (key, foot)
            if (depo, traj) == (2, 1):
                assert foot["Occupancy"] == 2, foot
            seen += 1
    assert seen == 6
