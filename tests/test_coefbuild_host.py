"""The device coefficient build's arithmetic (torj_coefbuild.hpp: cb_pivots, cb_prefilter_line,
cb_prof_node -- what k_coef_nodes and k_coef_prefilter run per lane) on the CPU: the host
build of tests/native/coefbuild_host.hip, looped over a whole plasma as the kernels' lanes
are, against the library's own host prefilters, `Plasma(...).coefs(k)`, bit for bit for all
six fields.  No tolerance: both are the same IEEE operation sequences.

The GPU test (tests/test_gpu_plasma_build.py) holds the kernels to the same coefficients."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_plasma_update_capi import FIELDS, fresh, tokamak_a, tokamak_b

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = C.POINTER(C.c_double)
NF = 8
SLOT = dict(Br=0, Bphi=1, Bz=2, lnne=3, lnTe=4, psi=5)  # torj_math.hpp Field


def load_harness():
    """libcoefbuild_host.so, compiled from tests/native/coefbuild_host.hip (host code only)."""
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", "libcoefbuild_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "coefbuild_host.hip")])
    L = C.CDLL(out)
    L.cb_build.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, _dp]
    L.cb_build.restype = None
    L.cb_line_differs.argtypes = [C.c_int, _dp]
    assert L.cb_nf() == NF
    return L


@pytest.fixture(scope="module")
def H():
    return load_harness()


def build(H, eq, f0=0, nf=6, coef=None):
    """the harness' interleaved coefficients of eq, (nZ + 2, nR + 2, NF)"""
    d = lambda a: a.ctypes.data_as(_dp)
    nR, nZ = len(eq["R_coords"]), len(eq["Z_coords"])
    m = [np.ascontiguousarray(np.asarray(eq[k], dtype=np.float64).T)
         for k in ("psi_norm_data", "Br_data", "Bz_data", "Bphi_data")]
    pr = [np.ascontiguousarray(eq[k], dtype=np.float64) for k in ("psi_prof", "ne_prof", "Te_prof")]
    if coef is None:
        coef = np.zeros((nZ + 2, nR + 2, NF))
    H.cb_build(nR, nZ, *[d(a) for a in m], len(pr[0]), *[d(a) for a in pr], f0, nf, d(coef))
    return coef


def assert_is_fresh(T, H, eq):
    P = fresh(T, eq)
    got = build(H, eq)
    for k in FIELDS:
        assert np.array_equal(got[..., SLOT[k]], P.coefs(k).T), k
    assert not got[..., 6:].any()  # the two spare doubles of a node stay zero


def tokamak(nR, nZ, **kw):
    from torj_hip import synthetic as S

    return S.circular_tokamak(nR=nR, nZ=nZ, **kw)


def test_slot_table(H):
    assert H.cb_slots_ok() == 1


@pytest.mark.parametrize("n", [2, 3, 4, 5, 31, 131])
def test_one_line(H, n):
    """cb_prefilter_line out of place against bspl1d_prefilter, n = 2 (no interior) and 3 (the first
    row is also the last) included"""
    y = np.random.default_rng(n).standard_normal(n) * 10.0 ** np.random.default_rng(n + 1).integers(-3, 4, n)
    assert H.cb_line_differs(n, y.ctypes.data_as(_dp)) == 0


@pytest.mark.parametrize("name", ["A", "B"])
def test_update_capi_plasmas(T, H, name):
    assert_is_fresh(T, H, dict(A=tokamak_a, B=tokamak_b)[name]())


@pytest.mark.parametrize("nR,nZ", [(2, 3), (3, 2), (3, 4), (4, 3), (70, 5)])
def test_small_and_odd_grids(T, H, nR, nZ):
    assert_is_fresh(T, H, tokamak(nR, nZ, n_prof=17, R_range=(1.05, 2.65), Z_range=(-0.85, 0.75)))


@pytest.mark.parametrize("n_prof", [2, 81])
def test_profile_lengths(T, H, n_prof):
    assert_is_fresh(T, H, tokamak(24, 31, n_prof=n_prof))


def test_non_uniform_psi_prof(T, H):
    eq = tokamak(24, 31)
    psi = np.linspace(0.0, 1.0, 41) ** 1.7
    assert np.ptp(np.diff(psi)) > 1e-3
    eq["psi_prof"] = psi
    eq["ne_prof"] = 3e19 * (1.0 - psi) + 1e17
    eq["Te_prof"] = 3000.0 * (1.0 - psi) ** 2 + 30.0
    assert_is_fresh(T, H, eq)


def test_nodes_outside_the_profile_range(T, H):
    """profiles over [0.05, 0.9]: nodes on both sides take the clamp and the Line() slope term"""
    eq = tokamak(24, 31)
    psi = np.linspace(0.05, 0.9, 33)
    eq["psi_prof"] = psi
    eq["ne_prof"] = 3e19 * (1.0 - psi) + 1e17
    eq["Te_prof"] = 3000.0 * (1.0 - psi) ** 2 + 30.0
    assert (eq["psi_norm_data"] < 0.05).any() and (eq["psi_norm_data"] > 0.9).any()
    assert_is_fresh(T, H, eq)


def test_profiles_only_build(T, H):
    """fields 1 and 2 alone on A's coefficients: A with B's profiles, the other four slots untouched"""
    from test_plasma_update_capi import with_profiles

    A, B = tokamak_a(), tokamak_b()
    AB = with_profiles(A, B)
    a = build(H, A)
    got = build(H, AB, f0=1, nf=2, coef=a.copy())
    P = fresh(T, AB)
    for k in FIELDS:
        assert np.array_equal(got[..., SLOT[k]], P.coefs(k).T), k
    for k in ("psi", "Br", "Bz", "Bphi"):
        assert np.array_equal(got[..., SLOT[k]], a[..., SLOT[k]]), k
    assert not np.array_equal(got[..., SLOT["lnne"]], a[..., SLOT["lnne"]])
