"""The register budget of the cell-tiled trajectory kernel:
k_traj_cell<2, true> (reference deposition with trajectory samples, the
headline's instance) compiled as csrc/Makefile compiles
torj_traj.hip must keep at most 176 VGPRs, no scratch and two waves per SIMD,
so that two trajectory waves and two 80-VGPR alpha waves share a SIMD.  The
figures are read from the footer of the kernel's assembly (no GPU needed)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_Z11k_traj_cellILi2ELb1EEv9TraceArgs9SplitArgs"


def test_k_traj_cell_resources(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import traj_isa_census as census
    finally:
        sys.path.pop(0)
    asm = str(tmp_path / "torj_traj.s")
    census.compile_asm([], asm)
    lines = open(asm).read().splitlines()
    name, body, rest = census.kernel_body(lines, KERNEL)
    assert name == KERNEL
    foot = {}
    for line in rest[:60]:
        m = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", line)
        if m and m.group(1) not in foot:
            foot[m.group(1)] = int(m.group(2))
    print(foot)
    assert foot["NumVgprs"] <= 176, foot
    assert foot["ScratchSize"] == 0, foot
    assert foot["Occupancy"] == 2, foot
    # the census reads the same assembly: the stage loop is found and is the
    # kernel's bulk
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "traj_isa_census.py"), "--asm", asm],
                         check=True, stdout=subprocess.PIPE, text=True).stdout
    tot = re.search(r"^loop total\s+(\d+)\s+(\d+)", out, re.M)
    assert tot and int(tot.group(1)) > 1000, out
