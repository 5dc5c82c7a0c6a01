"""The plan of a multi-beam launch through several plasmas (csrc/torj_launch.hpp
beams_plasmas_plan), host build, on CPU: the plasma index per beam, the plasmas'
records in listed order (one listed twice, one unused), the wave table equal to
beams_plan's for the same beam_off, and the argument checks the plasma form adds.
Every expected value is written by hand from the rules -- the records are the
listed plasmas' in order, beam b's index is beam_plasma[b], and the waves are those
of tests/test_beams_plan.py (beam b takes ceil(n_b / (64 / LPR)) waves) -- not
produced by the function under test."""
import ctypes as C
import math
import os
import subprocess

import pytest
from torj_hip._lib import TraceCfg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_ll = C.c_longlong
RAYS = 1
OM = 2 * math.pi * 92.5e9
# four listed plasmas: (device, coef tag, cellp tag, nR, nZ, psi_max); the tags stand for
# the device pointers a record carries.  Plasma 1 is listed again as plasma 3.
P_A = (0, 4096.0, 8192.0, 65, 65, 1.00)
P_B = (0, 12288.0, 16384.0, 72, 64, 1.25)
P_C = (0, 20480.0, 24576.0, 33, 129, 1.50)
LISTED = (P_A, P_B, P_C, P_B)


@pytest.fixture(scope="module")
def H():
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", "libbeams_plasmas_plan_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # libbeams_plan_host.so's flags (tests/test_beams_plan.py), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "beams_plasmas_plan_host.hip")])
    L = C.CDLL(out)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.bpp_plan.argtypes = [C.POINTER(TraceCfg), C.c_int, C.c_int, dp, C.c_int, ip, C.c_int, C.c_int, ip, dp, ip,
                           C.c_int, C.c_int, ip, C.POINTER(_ll), ip, dp, ip, ip, C.c_int]
    L.bpp_error.restype = C.c_char_p
    return L


def _arr(ty, v):
    return None if v is None else (ty * max(len(v), 1))(*v)


def plan(H, counts=(46, 5, 0, 1), beam_plasma=(0, 1, 3, 1), listed=LISTED, n_plasmas=None, null_list=False,
         device=0, absorption=1, integrator=0, sched_mode=-1, lanes_per_ray=0, n_cu=256):
    """beams_plasmas_plan -> dict (lpr, beam_pl, recs, waves, waves_ref: beams_plan's for
    the same beams), or the error text"""
    B = len(counts)
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    cfg = TraceCfg(0.0, 0, 1e-4, 100, 0, 1.0, 1e-6, absorption, 0, 0, integrator, 1e-6, 1e-6, 1.0, 100)
    kn = (C.c_int * 9)(n_cu, sched_mode, 0, lanes_per_ray, 1, 1, -1, 0, 0)
    flat = [float(v) for q in listed for v in q]
    out = (_ll * 7)()
    cap = 1 << 12
    beam_pl, recs = (C.c_int * max(B, 1))(), (C.c_double * (5 * max(len(listed), 1)))()
    waves, waves_ref = (C.c_int * (2 * cap))(), (C.c_int * (2 * cap))()
    rc = H.bpp_plan(C.byref(cfg), len(listed) if n_plasmas is None else n_plasmas, len(listed),
                    _arr(C.c_double, flat), int(null_list), _arr(C.c_int, beam_plasma), device, B,
                    _arr(C.c_int, off), _arr(C.c_double, [OM * (1 + b) for b in range(B)]),
                    _arr(C.c_int, [1, -1] * (B // 2) + [1] * (B % 2)), 0, RAYS, kn, out, beam_pl, recs, waves,
                    waves_ref, cap)
    if rc:
        assert rc == -1, "beams_plan alone refused what beams_plasmas_plan took"
        return H.bpp_error().decode()
    nw, nw_ref, n_rec, n_bpl = out[1], out[3], out[5], out[6]
    return dict(lpr=out[0], n=out[2], lpr_ref=out[4], beam_pl=[beam_pl[b] for b in range(n_bpl)],
                recs=[tuple(recs[5 * j + k] for k in range(5)) for j in range(n_rec)],
                waves=[(waves[2 * w], waves[2 * w + 1]) for w in range(nw)],
                waves_ref=[(waves_ref[2 * w], waves_ref[2 * w + 1]) for w in range(nw_ref)])


def test_plasma_index_and_records(H):
    """Four beams (46, 5, 0, 1 rays) through plasmas 0, 1, 3, 1 of four listed: plasma 1 is
    listed twice (as 1 and 3), plasma 2 is used by no beam.  The index is the caller's per
    beam, the empty beam's included; the records are the four listed, in listed order."""
    p = plan(H)
    assert p["beam_pl"] == [0, 1, 3, 1]
    assert p["recs"] == [(4096.0, 8192.0, 65, 65, 1.00), (12288.0, 16384.0, 72, 64, 1.25),
                         (20480.0, 24576.0, 33, 129, 1.50), (12288.0, 16384.0, 72, 64, 1.25)]
    assert p["n"] == 52


def test_wave_table_is_beams_plans(H):
    """The waves are beams_plan's for the same beam_off, whatever the plasmas: at 16 lanes
    per ray (4 rays per wave) 12 + 2 + 0 + 1 waves, at one lane per ray 1 + 1 + 0 + 1."""
    p = plan(H)
    assert (p["lpr"], p["lpr_ref"]) == (16, 16)
    want = [(0, 4 * j) for j in range(12)] + [(1, 46), (1, 50), (3, 51)]
    assert p["waves"] == want and p["waves_ref"] == want
    p = plan(H, lanes_per_ray=1)
    assert (p["lpr"], p["lpr_ref"]) == (1, 1)
    assert p["waves"] == [(0, 0), (1, 46), (3, 51)] == p["waves_ref"]
    # the lanes-per-ray rule on the whole launch, with the launching handle's knobs: 2048
    # padded waves fit two per SIMD on 256 CUs, 2049 do not -- one plasma or many
    assert plan(H, counts=(4,) * 2048, beam_plasma=(0, 1) * 1024)["lpr"] == 16
    assert plan(H, counts=(4,) * 2049, beam_plasma=(0, 1) * 1024 + (2,))["lpr"] == 1
    # one plasma for every beam: still beams_plan's table
    p = plan(H, beam_plasma=(0, 0, 0, 0), listed=(P_A,))
    assert p["waves"] == want and p["beam_pl"] == [0] * 4 and p["recs"] == [(4096.0, 8192.0, 65, 65, 1.00)]


def test_rejections(H):
    assert H.bpp_max_plasmas() == 4096
    assert plan(H, n_plasmas=0) == "n_plasmas must be 1..4096"
    assert plan(H, n_plasmas=4097) == "n_plasmas must be 1..4096"
    assert isinstance(plan(H, listed=(P_A,) * 4096, beam_plasma=(0, 4095, 7, 1)), dict)
    assert plan(H, null_list=True) == "plasmas is NULL"
    assert plan(H, beam_plasma=None) == "beam_plasma is NULL"
    assert plan(H, listed=(P_A, P_B, (-1, 0, 0, 0, 0, 0), P_B)) == "plasmas[2] is NULL"
    assert plan(H, beam_plasma=(0, -1, 3, 1)) == "beam_plasma[1] = -1 is outside 0..3 (n_plasmas = 4)"
    # (an empty beam's index is checked like any other)
    assert plan(H, beam_plasma=(0, 1, 4, 1)) == "beam_plasma[2] = 4 is outside 0..3 (n_plasmas = 4)"
    other = (1,) + P_C[1:]
    assert plan(H, listed=(P_A, P_B, other, P_B)) == \
        "plasmas[2] is on device 1, the launching handle on device 0 (one device per launch)"
    assert isinstance(plan(H, listed=(other,) * 4, device=1), dict)
    # beams_plan's own refusals come through unchanged
    assert plan(H, absorption=2) == \
        "absorption must be 0 or 1 in a multi-beam launch (the warm models trace one beam per call)"
    assert plan(H, integrator=1) == \
        "integrator must be 0 in a multi-beam launch (the adaptive integrator traces one beam per call)"
    for m in (1, 3):
        assert plan(H, sched_mode=m) == \
            f"sched mode {m} has no multi-beam form: only the one-shot kernel (torj_set_sched -1, 0, 2)"
