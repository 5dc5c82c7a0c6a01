"""The plan of a multi-beam launch (csrc/torj_launch.hpp beams_plan), host build,
on CPU: the argument checks, the lanes per ray and the wave table.  Every
expected value is worked out by hand from the rules -- beam b takes
ceil(n_b / (64 / LPR)) waves, wave j of a beam carries its rays (64 / LPR) j ...,
16 lanes per ray while the waves' 64 lanes each fit two waves per SIMD
(512 n_cu lanes) -- not produced by the function under test."""
import ctypes as C
import math
import os
import subprocess

import pytest
from torj_hip._lib import TraceCfg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_ll = C.c_longlong
OUT = ("lpr", "n_waves", "n", "depo", "fit", "tr", "DM", "n_save", "lay_bytes")
RAYS, GRID, DP, XL, S0, TRAJ = 1, 2, 4, 8, 16, 32
NONE, BINNED, SAMPLES = 0, 1, 2  # kDepoNone, kDepoBinned, kDepoSamples
OM = 2 * math.pi * 92.5e9


@pytest.fixture(scope="module")
def H():
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", "libbeams_plan_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # liblaunch_plan_host.so's flags (tests/test_launch_plan.py), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "beams_plan_host.hip")])
    L = C.CDLL(out)
    L.bp_plan.argtypes = [C.POINTER(TraceCfg), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double),
                          C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(_ll),
                          C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int]
    L.bp_error.restype = C.c_char_p
    return L


def _arr(ty, v):
    return None if v is None else (ty * len(v))(*v)


def plan(H, counts=(46,), omega=None, mode=None, beam_off="counts", n_beams=None, absorption=1, n_psi=0,
         has=RAYS, n_steps=100, integrator=0, deposition=0, traj_stride=0, ds=1e-4, n_cu=256, sched_mode=-1,
         lanes_per_ray=0, LPR=0, cfg_omega=0.0, cfg_mode=0):
    """beams_plan -> dict of the plan's fields, `waves` [(beam, first ray)] and
    `beams` [(lo, hi, mode, omega)], or the error text"""
    B = len(counts)
    if beam_off == "counts":
        beam_off = [0]
        for c in counts:
            beam_off.append(beam_off[-1] + c)
    omega = [OM] * B if omega is None else omega
    mode = [1] * B if mode is None else mode
    cfg = TraceCfg(cfg_omega, cfg_mode, ds, n_steps, 0, 1.0, 1e-6, absorption, traj_stride, deposition,
                   integrator, 1e-6, 1e-6, 1.0, 100)
    kn = (C.c_int * 9)(n_cu, sched_mode, 0, lanes_per_ray, 1, 1, -1, 0, LPR)
    out = (_ll * len(OUT))()
    cap = 1 << 16
    waves, beams, bom = (C.c_int * (2 * cap))(), (C.c_int * (3 * 8192))(), (C.c_double * 8192)()
    if H.bp_plan(C.byref(cfg), B if n_beams is None else n_beams, _arr(C.c_int, beam_off),
                 _arr(C.c_double, omega), _arr(C.c_int, mode), n_psi, has, kn, out, waves, cap, beams, bom, 8192):
        return H.bp_error().decode()
    p = dict(zip(OUT, out))
    p["waves"] = [(waves[2 * w], waves[2 * w + 1]) for w in range(p["n_waves"])]
    p["beams"] = [(beams[3 * b], beams[3 * b + 1], beams[3 * b + 2], bom[b]) for b in range(B)]
    return p


def rays_of(p, w):
    """rays wave w carries: up to its beam's end"""
    beam, first = p["waves"][w]
    return min(64 // p["lpr"], p["beams"][beam][1] - first)


BIN = dict(n_psi=1000, has=RAYS | GRID | DP)
FIT = dict(n_psi=1000, has=RAYS | GRID | DP | XL | S0, deposition=1)


def test_wave_table_16_lanes(H):
    """[46, 0, 1, 67] rays at 4 rays per wave: 12, 0, 1 and 17 waves"""
    p = plan(H, counts=(46, 0, 1, 67), omega=[OM, 2 * OM, 3 * OM, 4 * OM], mode=[1, -1, -1, 1])
    assert (p["lpr"], p["n_waves"], p["n"]) == (16, 30, 114)
    assert [b for b, _ in p["waves"]] == [0] * 12 + [2] + [3] * 17
    assert [f for _, f in p["waves"][:12]] == list(range(0, 48, 4))
    assert (p["waves"][11], rays_of(p, 11)) == ((0, 44), 2)
    assert (p["waves"][12], rays_of(p, 12)) == ((2, 46), 1)
    assert p["waves"][13] == (3, 47) and rays_of(p, 13) == 4
    assert (p["waves"][29], rays_of(p, 29)) == ((3, 111), 3)
    # the beams' records: ray ranges, and each beam's own frequency and mode
    assert p["beams"] == [(0, 46, 1, OM), (46, 46, -1, 2 * OM), (46, 47, -1, 3 * OM), (47, 114, 1, 4 * OM)]


def test_wave_table_one_lane(H):
    """the same beams at 64 rays per wave: 1, 0, 1 and 2 waves"""
    p = plan(H, counts=(46, 0, 1, 67), lanes_per_ray=1)
    assert (p["lpr"], p["n_waves"]) == (1, 4)
    assert p["waves"] == [(0, 0), (2, 46), (3, 47), (3, 111)]
    assert [rays_of(p, w) for w in range(4)] == [46, 1, 64, 3]


def test_lanes_threshold(H):
    """n_cu = 256: 2048 waves of 64 lanes fit two per SIMD, 2049 do not (a beam of 4
    rays is one wave at 16 lanes per ray; one of 5 rays is two)"""
    p = plan(H, counts=(4,) * 2048)
    assert (p["lpr"], p["n_waves"]) == (16, 2048)
    p = plan(H, counts=(4,) * 2049)
    assert (p["lpr"], p["n_waves"]) == (1, 2049)
    assert plan(H, counts=(5,) * 1024)["lpr"] == 16  # 2048 padded waves for 5120 rays
    assert plan(H, counts=(5,) * 1024 + (1,))["lpr"] == 1
    assert plan(H, counts=(4,) * 1216, n_cu=152)["lpr"] == 16
    assert plan(H, counts=(4,) * 1217, n_cu=152)["lpr"] == 1
    few = dict(counts=(4,) * 8)
    assert plan(H, **few)["lpr"] == 16
    assert plan(H, **few, **FIT)["lpr"] == 16
    assert plan(H, **few, **BIN)["lpr"] == 1
    assert plan(H, **few, absorption=0)["lpr"] == 1
    assert plan(H, **few, lanes_per_ray=1)["lpr"] == 1
    assert plan(H, **few, LPR=1)["lpr"] == 1
    assert plan(H, **few, lanes_per_ray=16, LPR=1)["lpr"] == 16
    assert plan(H, counts=(4,) * 2049, lanes_per_ray=16)["lpr"] == 16
    assert plan(H, counts=(4,) * 2049, lanes_per_ray=16, **BIN)["lpr"] == 1


def test_outputs(H):
    p = plan(H, counts=(46, 3), **FIT, n_steps=10)
    assert (p["depo"], p["fit"], p["DM"]) == (1, 1, SAMPLES)
    # the workspace of all 49 rays: one 64-ray block of 12 rows for the five per-step
    # arrays (no stored arc lengths), cnt 1001 x 49 ints and kstar 49 ints rounded to
    # 256 bytes, Fopen and dPs 1000 x 49 doubles
    assert p["lay_bytes"] == 5 * 64 * 12 * 8 + 196352 + 256 + 2 * 1000 * 49 * 8
    p = plan(H, counts=(46, 3), n_psi=1000, has=RAYS | GRID | DP | TRAJ, traj_stride=7)
    assert (p["depo"], p["fit"], p["DM"], p["tr"], p["n_save"]) == (1, 0, BINNED, 1, 14)
    p = plan(H, counts=(0, 0))  # nothing to trace is legal
    assert (p["n"], p["n_waves"]) == (0, 0)
    # cfg's own omega and mode are ignored
    assert isinstance(plan(H, cfg_omega=float("nan"), cfg_mode=7), dict)


def test_rejections(H):
    cap = H.bp_max_beams()
    assert cap == 4096
    assert plan(H, counts=(), n_beams=0, beam_off=[0]) == "n_beams must be 1..4096"
    assert plan(H, counts=(1,) * (cap + 1)) == "n_beams must be 1..4096"
    assert isinstance(plan(H, counts=(1,) * cap), dict)
    assert plan(H, beam_off=None) == "beam_off is NULL"
    assert plan(H, beam_off=[1, 47]) == "beam_off[0] must be 0"
    assert plan(H, counts=(4, 4, 4), beam_off=[0, 4, 3, 12]) == "beam_off must not decrease (beam 1)"
    for bad in (0.0, -OM, float("nan"), float("inf")):
        assert plan(H, counts=(4, 4), omega=[OM, bad]) == "omega[1] must be finite and > 0"
    for bad in (0, 2, -2):
        assert plan(H, counts=(4, 4, 4), mode=[1, -1, bad]) == "mode[2] must be +1 (X) or -1 (O)"
    assert plan(H, has=GRID | DP | XL | S0 | TRAJ) == "x0, N0, state, status, steps required"
    assert plan(H, n_steps=-1) == "n_steps < 0"
    assert plan(H, ds=0.0) == "ds must be > 0"
    assert plan(H, ds=float("nan")) == "ds must be > 0"
    assert plan(H, deposition=2) == "deposition must be 0 or 1"
    warm = "absorption must be 0 or 1 in a multi-beam launch (the warm models trace one beam per call)"
    for a in (-1, 2, 3, 4):
        assert plan(H, absorption=a) == warm
    assert plan(H, integrator=1) == \
        "integrator must be 0 in a multi-beam launch (the adaptive integrator traces one beam per call)"
    for m in (1, 3):
        assert plan(H, sched_mode=m) == \
            f"sched mode {m} has no multi-beam form: only the one-shot kernel (torj_set_sched -1, 0, 2)"
    assert isinstance(plan(H, sched_mode=0), dict)
    fit = "deposition = 1 (reference profile) needs x_launch and s0 (torj_trace_ex)"
    assert plan(H, n_psi=5, has=RAYS | GRID | DP | XL, deposition=1) == fit
    assert plan(H, n_psi=5, has=RAYS | GRID | DP | S0, deposition=1) == fit
    assert isinstance(plan(H, n_psi=5, has=RAYS | GRID | XL, deposition=1), dict)  # no dP: no deposition
