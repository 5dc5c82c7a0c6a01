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
    return L


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
