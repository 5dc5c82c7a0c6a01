"""torj_plasma_update_gpu, torj_plasma_update_profiles_gpu, torj_plasma_update_device at the
C-ABI boundary (include/torj_hip.h), host side: the symbols, and every refusal -- a NULL or
too-short argument by name, a profiles-only call on a handle whose equilibrium came as
coefficients, no usable GPU -- which leaves the handle, in every host result, as it was.

The handles here sit on device 7777, which no machine has: the calls that pass the argument
checks are refused for want of a GPU with and without one in the machine.  What the calls
compute is tests/test_gpu_plasma_build.py's."""
import ctypes

import numpy as np
import pytest

from test_plasma_update_capi import (assert_same, coefs_args, host_results, tokamak_a, tokamak_b)

NEW = ("torj_plasma_update_gpu", "torj_plasma_update_profiles_gpu", "torj_plasma_update_device")
NO_DEVICE = 7777
MAPS = ("psi_norm_data", "Br_data", "Bz_data", "Bphi_data")


@pytest.fixture(scope="module")
def AB():
    return tokamak_a(), tokamak_b()


def handle(T, eq):
    from torj_hip import synthetic as S

    return T.Plasma(*S.plasma_args(eq), device=NO_DEVICE)


def _raw_full(T, fn, h, eq, **kw):
    """torj_plasma_update_gpu / _device on eq's host arrays (for _device the refusals come before any
    read of the maps, so host pointers stand in for device pointers)"""
    d = T._lib.dptr
    m = {k: np.ascontiguousarray(np.asarray(eq[k], dtype=np.float64).T) for k in MAPS}
    if fn == "torj_plasma_update_device":
        mp = {k: m[k].ctypes.data for k in MAPS}
    else:
        mp = {k: d(m[k]) for k in MAPS}
    a = dict(p=h, R_coords=d(eq["R_coords"]), Z_coords=d(eq["Z_coords"]), psi_norm_data=mp["psi_norm_data"],
             n_prof=len(eq["psi_prof"]), psi_prof=d(eq["psi_prof"]), ne_prof=d(eq["ne_prof"]),
             Te_prof=d(eq["Te_prof"]), Br_data=mp["Br_data"], Bz_data=mp["Bz_data"], Bphi_data=mp["Bphi_data"],
             n_eq=len(eq["eqt1d_psi_norm"]), eqt1d_psi_norm=d(eq["eqt1d_psi_norm"]),
             eqt1d_volume=d(eq["eqt1d_volume"]))
    a.update(kw)
    rc = getattr(T.lib(), fn)(*a.values(), None)
    return rc, T.lib().torj_last_error().decode()


def _raw_profiles(T, h, eq, **kw):
    d = T._lib.dptr
    a = dict(p=h, n_prof=len(eq["psi_prof"]), psi_prof=d(eq["psi_prof"]), ne_prof=d(eq["ne_prof"]),
             Te_prof=d(eq["Te_prof"]))
    a.update(kw)
    rc = T.lib().torj_plasma_update_profiles_gpu(*a.values(), None)
    return rc, T.lib().torj_last_error().decode()


def test_symbols_exported(T):
    L = ctypes.CDLL(T.LIB_PATH)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in T.EXPORTED
    assert T.lib().torj_abi_version() == 8  # symbols added, nothing changed


def test_refusals_name_the_argument_and_leave_the_handle(T, AB):
    A, B = AB
    P = handle(T, A)
    h = P.handle
    before = host_results(T, P)
    cases = []
    for fn in ("torj_plasma_update_gpu", "torj_plasma_update_device"):
        cases.append((_raw_full(T, fn, None, B), f"{fn}: p is NULL"))
        for name in ("R_coords", "Z_coords", "psi_norm_data", "psi_prof", "ne_prof", "Te_prof", "Br_data", "Bz_data",
                     "Bphi_data", "eqt1d_psi_norm", "eqt1d_volume"):
            cases.append((_raw_full(T, fn, h, B, **{name: None}), f"{fn}: {name} is NULL"))
        cases.append((_raw_full(T, fn, h, B, n_prof=1), f"{fn}: n_prof = 1 < 2"))
        cases.append((_raw_full(T, fn, h, B, n_eq=0), f"{fn}: n_eq = 0 < 2"))
    fn = "torj_plasma_update_profiles_gpu"
    cases.append((_raw_profiles(T, None, B), f"{fn}: p is NULL"))
    for name in ("psi_prof", "ne_prof", "Te_prof"):
        cases.append((_raw_profiles(T, h, B, **{name: None}), f"{fn}: {name} is NULL"))
    cases.append((_raw_profiles(T, h, B, n_prof=-3), f"{fn}: n_prof = -3 < 2"))
    for (rc, msg), text in cases:
        assert rc != 0 and msg == text, (msg, text)
    assert_same(host_results(T, P), before)


def test_without_a_gpu_the_calls_fail(T, AB):
    A, B = AB
    P = handle(T, A)
    before = host_results(T, P)
    for fn in ("torj_plasma_update_gpu", "torj_plasma_update_device"):
        rc, msg = _raw_full(T, fn, P.handle, B)
        assert rc != 0 and msg.startswith(f"{fn}: no usable GPU for the handle"), msg
    rc, msg = _raw_profiles(T, P.handle, B)
    assert rc != 0 and msg.startswith("torj_plasma_update_profiles_gpu: no usable GPU for the handle"), msg
    assert_same(host_results(T, P), before)
    # the wrappers raise it
    from torj_hip import synthetic as S

    with pytest.raises(T.TorjError, match="no usable GPU"):
        P.update_gpu(*S.plasma_args(B))
    with pytest.raises(T.TorjError, match="no usable GPU"):
        P.update_profiles_gpu(B["psi_prof"], B["ne_prof"], B["Te_prof"])
    assert_same(host_results(T, P), before)
    assert (P.R_coords[0], P.R_coords[-1]) == (A["R_coords"][0], A["R_coords"][-1])
    # the host update still goes through on the same handle
    P.update(*S.plasma_args(B))
    assert_same(host_results(T, P), host_results(T, handle(T, B)))


def test_profiles_call_on_a_from_coefs_handle_is_refused(T, AB):
    A, B = AB
    P = T.Plasma.from_coefs(*coefs_args(T, A), device=NO_DEVICE)
    before = host_results(T, P)
    rc, msg = _raw_profiles(T, P.handle, B)
    assert rc != 0
    assert msg.startswith("torj_plasma_update_profiles_gpu: the handle has no psi_norm_data"), msg
    assert_same(host_results(T, P), before)


def test_wrappers_keep_the_grid_size(T, AB):
    from torj_hip import synthetic as S
    from test_plasma_update_capi import NR, NZ

    P = handle(T, AB[0])
    bad = S.plasma_args(S.circular_tokamak(nR=NR + 1, nZ=NZ))
    with pytest.raises(ValueError, match="grid size"):
        P.update_gpu(*bad)
    with pytest.raises(ValueError, match="grid size"):
        P.update_device(bad[0], bad[1], 1, bad[3], bad[4], bad[5], 1, 1, 1, bad[9], bad[10])
