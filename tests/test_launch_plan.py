"""The launch plan of one trace call (csrc/torj_launch.hpp launch_plan), the
reference deposition's workspace (fit_layout, fit_bytes_per_ray) and the batch
size (batch_rays), host build, on CPU.  Every expected value is worked out by
hand from the rules the library had before the plan existed (G = ceil(n / 64)
groups; the queue by default for G > 4 n_cu; the fully relativistic model splits
for G < 3 n_cu; 16 lanes per ray while 16 n <= 512 n_cu lanes), not produced by
the function under test."""
import ctypes as C
import os
import subprocess

import pytest
from torj_hip._lib import TraceCfg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_ll = C.c_longlong
OUT = ("path", "depo", "fit", "tr", "adaptive", "DM", "n_save", "G", "cs", "W", "S", "ctl_bytes", "lds",
       "hist_off", "n_hist", "grid", "lay_bytes")
RAYS, GRID, DP, XL, S0, TRAJ = 1, 2, 4, 8, 16, 32
NONE, BINNED, SAMPLES = 0, 1, 2  # kDepoNone, kDepoBinned, kDepoSamples


@pytest.fixture(scope="module")
def H():
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", "liblaunch_plan_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # libh3_fast_host.so's flags (tests/test_h3_fast_host.py), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "launch_plan_host.hip")])
    L = C.CDLL(out)
    L.lp_plan.argtypes = [C.POINTER(TraceCfg), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(_ll)]
    L.lp_error.restype = C.c_char_p
    L.lp_fit_layout.argtypes = [_ll, _ll, _ll, C.c_int, C.POINTER(_ll)]
    L.lp_fit_bytes_per_ray.argtypes = [_ll, _ll, C.c_int]
    L.lp_fit_bytes_per_ray.restype = _ll
    L.lp_batch_rays.argtypes = [_ll, _ll, _ll, C.c_long]
    L.lp_batch_rays.restype = _ll
    c = (C.c_int * 6)()
    L.lp_consts(c)
    L.SPLIT, L.QUEUE, L.LANE1, L.LANE16, L.kTsLds, L.kSplitMaxSteps = list(c)
    return L


def plan(H, absorption=1, n=64, n_psi=0, has=RAYS, n_steps=100, integrator=0, deposition=0, traj_stride=0,
         chunk_steps=0, mode=1, ds=1e-4, s_max=0.0, n_chunks=100, abstol=1e-6, reltol=1e-6, n_cu=256,
         sched_mode=-1, sched_waves=0, lanes_per_ray=0, SCHED=1, SPLIT=1, SPLIT_WARM=-1, SCHED_W=0, LPR=0):
    """launch_plan -> dict of the plan's fields, or the error text"""
    cfg = TraceCfg(2 * 3.141592653589793 * 92.5e9, mode, ds, n_steps, chunk_steps, 1.0, 1e-6, absorption,
                   traj_stride, deposition, integrator, abstol, reltol, s_max, n_chunks)
    kn = (C.c_int * 9)(n_cu, sched_mode, sched_waves, lanes_per_ray, SCHED, SPLIT, SPLIT_WARM, SCHED_W, LPR)
    out = (_ll * len(OUT))()
    if H.lp_plan(C.byref(cfg), n, n_psi, has, kn, out):
        return H.lp_error().decode()
    return dict(zip(OUT, out))


BIN = dict(n_psi=1000, has=RAYS | GRID | DP)  # binned deposition
FIT = dict(n_psi=1000, has=RAYS | GRID | DP | XL | S0, deposition=1)


def test_lanes(H):
    """16 lanes per ray: Albajar without binned deposition while 16 n <= 512 n_cu"""
    p = plan(H, n=8192)
    assert (p["path"], p["grid"], p["DM"]) == (H.LANE16, 512, NONE)
    assert plan(H, n=8193)["path"] == H.LANE1
    assert plan(H, n=8192, **BIN)["path"] == H.LANE1
    assert plan(H, n=8192, **FIT)["path"] == H.LANE16
    assert plan(H, n=8192, absorption=0)["path"] == H.LANE1
    assert plan(H, n=8192, lanes_per_ray=1)["path"] == H.LANE1
    assert plan(H, n=8192, LPR=1)["path"] == H.LANE1
    p = plan(H, n=20000, lanes_per_ray=16)
    assert (p["path"], p["grid"]) == (H.LANE16, 1250)
    assert plan(H, n=20000, lanes_per_ray=16, **BIN)["path"] == H.LANE1
    assert plan(H, n=20000, lanes_per_ray=16, LPR=1)["path"] == H.LANE16
    p = plan(H, n=65536)  # G = 1024: not more than 4 n_cu
    assert (p["path"], p["grid"], p["G"]) == (H.LANE1, 256, 1024)


def test_albajar_and_cold_thresholds(H):
    """G > 4 n_cu: Albajar splits (TORJ_SPLIT=0: queues), the cold model queues"""
    assert plan(H, n=65600)["path"] == H.SPLIT  # G = 1025
    p = plan(H, n=65600, SPLIT=0)
    assert (p["path"], p["G"], p["W"], p["S"], p["ctl_bytes"]) == (H.QUEUE, 1025, 961, 7944, 63808)
    assert (p["cs"], p["hist_off"], p["n_hist"], p["lds"]) == (100, 0, 0, 0)
    p = plan(H, n=70000, absorption=0)  # G = 1094, W = G - G / 16
    assert (p["path"], p["W"]) == (H.QUEUE, 1026)
    assert plan(H, n=65600, SCHED=0)["path"] == H.LANE1
    assert plan(H, n=70000, absorption=0, SCHED=0)["path"] == H.LANE1
    assert plan(H, n=65600, n_cu=304)["path"] == H.LANE1  # 1025 <= 1216
    assert plan(H, n=65600, SPLIT=0, chunk_steps=20)["cs"] == 20


def test_warm(H):
    """the warm models never take a one-shot kernel with steps to do: weakly
    relativistic splits, fully relativistic splits below 3 groups per CU"""
    assert plan(H, absorption=2, n=64)["path"] == H.SPLIT
    assert plan(H, absorption=2, n=100000)["path"] == H.SPLIT
    assert plan(H, absorption=3, n=49088)["path"] == H.SPLIT  # G = 767
    p = plan(H, absorption=3, n=49089)  # G = 768; one wave per SIMD, G - G / 16
    assert (p["path"], p["G"], p["W"]) == (H.QUEUE, 768, 720)
    assert plan(H, absorption=3, n=49089, SPLIT_WARM=1)["path"] == H.SPLIT
    assert plan(H, absorption=3, n=49088, SPLIT_WARM=0)["path"] == H.QUEUE
    assert plan(H, absorption=2, n=64, SPLIT_WARM=0)["path"] == H.QUEUE
    assert plan(H, absorption=2, n=64, SPLIT=0)["path"] == H.QUEUE
    assert plan(H, absorption=3, n=64, sched_mode=0)["path"] == H.QUEUE
    assert plan(H, absorption=3, n=200000)["W"] == 1024  # 4 n_cu TORJ_WARM_MIN_WAVES


@pytest.mark.parametrize("absorption", [0, 1, 2, 3])
def test_adaptive(H, absorption):
    """integrator 1: the queue, never split; the stage vectors take the LDS"""
    for kw in (dict(), dict(sched_mode=3), dict(sched_mode=0), BIN, dict(n=100000)):
        p = plan(H, absorption=absorption, integrator=1, s_max=0.5, **kw)
        assert (p["path"], p["adaptive"], p["hist_off"], p["n_hist"]) == (H.QUEUE, 1, H.kTsLds, 0), kw
        assert p["lds"] == 8 * H.kTsLds


def test_queue_histogram(H):
    """binned shells on the RK4 queue: an LDS histogram up to 4096 shells"""
    kw = dict(n=70000, absorption=0, has=RAYS | GRID | DP)
    p = plan(H, n_psi=4096, **kw)
    assert (p["path"], p["DM"], p["n_hist"], p["hist_off"], p["lds"]) == (H.QUEUE, BINNED, 4096, 0, 32768)
    assert plan(H, n_psi=4097, **kw)["n_hist"] == 0
    p = plan(H, n=70000, absorption=0, **FIT)
    assert (p["DM"], p["n_hist"]) == (SAMPLES, 0)


def test_sched_modes(H):
    assert plan(H, sched_mode=3)["path"] == H.SPLIT  # Albajar, 64 rays
    assert plan(H, sched_mode=3, absorption=0)["path"] == H.QUEUE  # any non-zero mode is "queue on"
    # no steps: nothing to queue or split, the one-shot kernel (warm: its cold instance);
    # a small Albajar beam is still spread over 16 lanes per ray there
    assert plan(H, sched_mode=3, absorption=0, n_steps=0)["path"] == H.LANE1
    assert plan(H, sched_mode=3, absorption=3, n_steps=0)["path"] == H.LANE1
    assert plan(H, sched_mode=3, absorption=1, n_steps=0)["path"] == H.LANE16
    assert plan(H, absorption=2, n_steps=0)["path"] == H.LANE1
    assert 1 << 24 == H.kSplitMaxSteps
    assert plan(H, sched_mode=3, n_steps=1 << 24)["path"] == H.QUEUE
    assert plan(H, sched_mode=3, n_steps=(1 << 24) - 1)["path"] == H.SPLIT
    assert plan(H, sched_mode=3, SPLIT=0, SCHED=0)["path"] == H.SPLIT  # the handle's mode beats the environment
    assert plan(H, sched_mode=0, n=65600)["path"] == H.LANE1
    p = plan(H, sched_mode=1, sched_waves=3, n=64 * 3)
    assert (p["path"], p["G"], p["W"], p["S"]) == (H.QUEUE, 3, 3, 24)
    assert plan(H, sched_mode=1, sched_waves=3, n=100000)["W"] == 3
    p = plan(H, sched_mode=1, sched_waves=50, n=640)  # G = 10
    assert (p["G"], p["W"]) == (10, 10)
    assert plan(H, sched_mode=1, SCHED_W=7, n=6400)["W"] == 7
    assert plan(H, sched_mode=1, SCHED_W=7, sched_waves=5, n=6400)["W"] == 5
    assert plan(H, sched_mode=1, n=64)["W"] == 1  # G - G / 16 = 1


def test_outputs(H):
    p = plan(H, n=100, has=RAYS | TRAJ, traj_stride=7)
    assert (p["tr"], p["n_save"], p["depo"], p["fit"]) == (1, 14, 0, 0)
    assert plan(H, n=100, has=RAYS, traj_stride=7)["tr"] == 0
    assert plan(H, n=100, has=RAYS | TRAJ)["n_save"] == 0
    p = plan(H, n=100, n_psi=5, has=RAYS | GRID | DP | XL | S0, deposition=1, n_steps=10)
    assert (p["depo"], p["fit"], p["DM"], p["lay_bytes"]) == (1, 1, SAMPLES, 72512)
    p = plan(H, n=100, n_psi=5, has=RAYS | GRID | DP | XL | S0, deposition=1, n_steps=10, integrator=1, s_max=1.0)
    assert p["lay_bytes"] == 84800
    assert plan(H, n=100, n_psi=1, has=RAYS | GRID | DP)["depo"] == 0
    assert plan(H, n=100, n_psi=5, has=RAYS | GRID)["depo"] == 0


def test_argument_errors(H):
    """the texts and their order"""
    bad = dict(has=0, n_steps=-1, mode=0, ds=0.0, deposition=2, integrator=2, absorption=4)
    order = [("has", "x0, N0, state, status, steps required"), ("n_steps", "n_steps < 0"),
             ("mode", "mode must be +1 (X) or -1 (O)"), ("ds", "ds must be > 0"),
             ("deposition", "deposition must be 0 or 1"), ("integrator", "integrator must be 0 or 1"),
             ("absorption", "absorption must be 0..3")]
    for key, text in order:
        assert plan(H, **bad) == text
        del bad[key]
    assert isinstance(plan(H, **bad), dict)
    assert plan(H, has=GRID | DP | XL | S0 | TRAJ) == "x0, N0, state, status, steps required"
    assert plan(H, ds=float("nan")) == "ds must be > 0"
    assert plan(H, absorption=-1) == "absorption must be 0..3"
    need = "integrator 1 needs s_max > 0, n_chunks >= 1, abstol, reltol > 0, n_steps >= 1"
    for kw in (dict(s_max=0.0), dict(n_chunks=0), dict(abstol=0.0), dict(reltol=0.0), dict(n_steps=0)):
        assert plan(H, integrator=1, **{"s_max": 1.0, **kw}) == need
    fit = "deposition = 1 (reference profile) needs x_launch and s0 (torj_trace_ex)"
    assert plan(H, n_psi=5, has=RAYS | GRID | DP | XL, deposition=1) == fit
    assert plan(H, n_psi=5, has=RAYS | GRID | DP | S0, deposition=1) == fit
    assert plan(H, n_psi=5, has=RAYS | GRID | DP | S0, deposition=1, absorption=4) == fit  # before the model's check
    assert isinstance(plan(H, n_psi=5, has=RAYS | GRID | XL, deposition=1), dict)  # no dP: no deposition


def test_fit_layout(H):
    """n = 100 (two 64-ray blocks), 12 rows, 5 boundaries: per-step arrays of
    128 * 12 doubles, cnt 6 * 100 ints and kstar 100 ints rounded to 256 bytes"""
    off = (_ll * 11)()
    H.lp_fit_layout(100, 12, 5, 0, off)
    KN = 128 * 12 * 8
    assert list(off) == [0, KN, 2 * KN, 2 * KN, 3 * KN, 4 * KN, 61440, 64000, 68000, 72000, 72512]
    assert off[3] == 24576  # E
    assert H.lp_fit_bytes_per_ray(12, 5, 0) == 588  # 5 * 8 * 12 + 4 * 6 + 16 * 5 + 4
    H.lp_fit_layout(100, 12, 5, 1, off)
    assert list(off) == [0, KN, 2 * KN, 3 * KN, 4 * KN, 5 * KN, 61440 + KN, 64000 + KN, 68000 + KN, 72000 + KN, 84800]
    assert KN == 12288
    assert H.lp_fit_bytes_per_ray(12, 5, 1) == 588 + 96
    # the headline shape: 2000 steps, 1000 shells
    assert H.lp_fit_bytes_per_ray(2002, 1000, 0) == 5 * 8 * 2002 + 4 * 1001 + 16 * 1000 + 4


def test_batch_rays(H):
    per_ray = H.lp_fit_bytes_per_ray(12, 5, 0)
    assert H.lp_batch_rays(100, per_ray, 30000, 0) == 64  # 51 rays fit: one group at least
    assert H.lp_batch_rays(1000, per_ray, 100000, 0) == 128  # 170 rays fit
    assert H.lp_batch_rays(1000, per_ray, 10 ** 6, 0) == 1000
    assert H.lp_batch_rays(1000, 0, 0, 0) == 1000  # no reference deposition: no budget
    assert H.lp_batch_rays(1000, 0, 0, 256) == 256  # TORJ_SPLIT_BATCH
    assert H.lp_batch_rays(1000, per_ray, 100000, 256) == 128
    assert H.lp_batch_rays(1000, per_ray, 100000, 64) == 64
