"""The group flag words in the split pipeline's launch plan (csrc/torj_split.hpp
split_plan_sizes and split_carve), host build, on CPU: one unsigned per 64-ray
group for each of the kRing ring slots, each slot's array rounded up to 256
bytes and 256-byte aligned (no two slots share a cache line); none when
TORJ_ALPHA_GFLAG=0, when TORJ_ALPHA_ZFLAG=0, for a warm model or without the
early settle.  Every expected size is written from that rule."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BASE = 1 << 32  # a 256-byte-aligned stand-in for the workspace's address
KNOBS = ("TORJ_ALPHA_GFLAG", "TORJ_ALPHA_ZFLAG")


@pytest.fixture(scope="module")
def H():
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", "libsplit_plan_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # libbeams_plasmas_plan_host.so's flags (tests/test_beams_plasmas_plan.py), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "split_plan_host.hip")])
    L = C.CDLL(out)
    L.spl_plan.argtypes = [C.c_longlong] + [C.c_int] * 9 + [C.c_ulonglong, C.c_ulonglong,
                                                           C.POINTER(C.c_ulonglong)]
    L.spl_traj_mode.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_ulonglong)]
    return L


def traj_mode(H, n, nR, nZ, lds):
    """(the trajectory kernel the plan picks for n rays on an nR x nZ grid under
    TORJ_TRAJ_LDS = lds: 0 k_traj, 1 k_traj_lds, 2 k_traj_tile, 3 k_traj_cell; k_traj_lds'
    dynamic LDS bytes on that grid)"""
    old = os.environ.get("TORJ_TRAJ_LDS")
    try:
        if lds is None:
            os.environ.pop("TORJ_TRAJ_LDS", None)
        else:
            os.environ["TORJ_TRAJ_LDS"] = lds
        b = C.c_ulonglong(0)
        return H.spl_traj_mode(n, nR, nZ, C.byref(b)), b.value
    finally:
        if old is None:
            os.environ.pop("TORJ_TRAJ_LDS", None)
        else:
            os.environ["TORJ_TRAJ_LDS"] = old


def test_trajectory_kernel_in_the_plan(H):
    """TORJ_TRAJ_LDS picks the trajectory kernel (split_traj_mode): the cell tile by
    default, and with 1 the whole-grid LDS kernel only while 48 B for each of the
    (nR + 2)(nZ + 2) coefficients fit 160 KiB -- the 56 x 56 grid (161 472 B) and the
    40 x 61 grid of tests/shaped_eq.py (127 008 B) do, 57 x 57 (167 088 B) and 129 x 129
    do not and fall back to the L2 kernel."""
    import shaped_eq as E

    assert traj_mode(H, 187, 56, 56, None)[0] == 3
    for lds in ("0", "2", "3"):
        assert traj_mode(H, 187, E.NR, E.NZ, lds) == (int(lds), 42 * 63 * 48)
    assert traj_mode(H, 187, E.NR, E.NZ, "1") == (1, 127008)
    assert traj_mode(H, 100203, 56, 56, "1") == (1, 58 * 58 * 48)
    assert 58 * 58 * 48 <= 160 * 1024 < 59 * 59 * 48
    assert traj_mode(H, 187, 57, 57, "1") == (0, 59 * 59 * 48)
    assert traj_mode(H, 187, 129, 129, "1")[0] == 0
    assert traj_mode(H, 187, 129, 129, "3")[0] == 3


def plan(H, n, env=None, abs_model=1, counted=0, depo=2, walk=1, negl_skip=1, n_steps=2000, chunk=20,
         sched=(3, 20)):
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env or {})
        out = (C.c_ulonglong * 32)()
        k = H.spl_plan(n, n_steps, chunk, abs_model, counted, depo, walk, negl_skip, sched[0], sched[1],
                       64 << 30, BASE, out)
    finally:
        for key, v in old.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v
    R = out[5]
    assert k == 8 + 2 * R + 1
    return dict(bytes=out[0], b_gf=out[1], b_zf=out[2], zflag_on=out[3], gflag_on=out[4], R=R, kb=out[6],
                n_blk=out[7], zflags=list(out[8:8 + R]), gflags=list(out[8 + R:8 + 2 * R]), end=out[8 + 2 * R])


def al(b):
    return (b + 255) // 256 * 256


# one ray, one group, a ragged last group, exactly 64 groups (one 256-byte array), one
# group more, and the headline beam's 100 203 rays
@pytest.mark.parametrize("n", [1, 64, 229, 4096, 4097, 100203])
@pytest.mark.parametrize("counted,depo,walk", [(0, 2, 1), (1, 1, 0), (0, 0, 0)])
def test_group_words_in_the_plan(H, n, counted, depo, walk):
    kw = dict(counted=counted, depo=depo, walk=walk)
    on, off = plan(H, n, **kw), plan(H, n, {"TORJ_ALPHA_GFLAG": "0"}, **kw)
    groups = (n + 63) // 64
    assert on["R"] == 4
    assert (on["zflag_on"], on["gflag_on"]) == (1, 1) and (off["zflag_on"], off["gflag_on"]) == (1, 0)
    # exactly kRing arrays of al(4 * ceil(n / 64)) bytes more, nothing else moved in size
    assert on["b_gf"] == al(4 * groups) and off["b_gf"] == 0
    assert on["bytes"] - off["bytes"] == on["R"] * al(4 * groups)
    assert (on["kb"], on["n_blk"]) == (off["kb"], off["n_blk"]) == (20, 100)
    # the carve hands out every byte of the plan, with and without the words
    assert on["end"] - BASE == on["bytes"] and off["end"] - BASE == off["bytes"]
    # every slot's array 256-byte aligned, one array apart, behind the per-ray flags
    g = on["gflags"]
    assert all(p != 0 and p % 256 == 0 for p in g)
    assert [g[r + 1] - g[r] for r in range(on["R"] - 1)] == [al(4 * groups)] * (on["R"] - 1)
    assert g[0] == on["zflags"][-1] + al(n)
    assert all(p % 256 == 0 for p in on["zflags"]) and on["zflags"] == off["zflags"]
    # off: the pointers are null
    assert off["gflags"] == [0] * off["R"]


@pytest.mark.parametrize("env,kw", [({"TORJ_ALPHA_ZFLAG": "0"}, {}),
                                    ({"TORJ_ALPHA_ZFLAG": "0", "TORJ_ALPHA_GFLAG": "1"}, {}),
                                    ({}, {"negl_skip": 0}), ({}, {"abs_model": 2}), ({}, {"abs_model": 3})])
def test_no_group_words_without_zero_flags(H, env, kw):
    """TORJ_ALPHA_ZFLAG=0 implies no group words, whatever TORJ_ALPHA_GFLAG says; so do
    the warm models and a quadrature table without the early settle."""
    p = plan(H, 229, env, **kw)
    assert (p["zflag_on"], p["gflag_on"], p["b_zf"], p["b_gf"]) == (0, 0, 0, 0)
    assert p["zflags"] == [0] * p["R"] and p["gflags"] == [0] * p["R"]
    assert p["end"] - BASE == p["bytes"]
    q = plan(H, 229, dict(env, TORJ_ALPHA_GFLAG="0"), **kw)
    assert q["bytes"] == p["bytes"]
