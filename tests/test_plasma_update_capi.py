"""torj_plasma_update, torj_plasma_update_from_coefs, torj_plasma_update_profiles at the
C-ABI boundary (include/torj_hip.h), host side: without a GPU the update is host-only, and
a handle updated to a plasma is in every host result bit for bit a fresh handle of that
plasma.  Every refusal names its argument and leaves the handle as it was.

Two synthetic tokamaks on 24 x 31 nodes: A, and B with Te0 = 6000, ne_scale = 0.6, another
box, other profile and volume tables."""
import ctypes

import numpy as np
import pytest

NR, NZ = 24, 31
OM = 2 * np.pi * 92.5e9
FIELDS = ("psi", "lnne", "lnTe", "Br", "Bz", "Bphi")
NEW = ("torj_plasma_update", "torj_plasma_update_from_coefs", "torj_plasma_update_profiles",
       "torj_plasma_get_cell_table")


def tokamak_a():
    from torj_hip import synthetic as S

    return S.circular_tokamak(nR=NR, nZ=NZ)


def tokamak_b():
    from torj_hip import synthetic as S

    eq = S.circular_tokamak(nR=NR, nZ=NZ, Te0=6000, ne_scale=0.6, n_prof=81, R_range=(1.05, 2.65),
                            Z_range=(-0.85, 0.75))
    psi = np.linspace(0.0, 1.2, 77)
    eq["eqt1d_psi_norm"] = psi
    eq["eqt1d_volume"] = 2.0 * np.pi ** 2 * S.R0 * S.A_MINOR ** 2 * psi ** 1.1
    return eq


def with_profiles(eq, prof):
    """eq's maps and volume table, prof's kinetic profiles"""
    out = dict(eq)
    for k in ("psi_prof", "ne_prof", "Te_prof"):
        out[k] = prof[k]
    return out


def fresh(T, eq):
    from torj_hip import synthetic as S

    return T.Plasma(*S.plasma_args(eq))


def default_fan(T):
    N0 = T.pol_tor_angles_2_vector(np.deg2rad(30.0), 0.0)
    pos, dirs, w = T.launch_peripheral_rays([2.5, 0, 0.4], N0, 0.0174, 1 / 3.99, 92.5e9)
    assert len(w) == 46
    return pos, dirs, w


def host_results(T, P):
    """everything the host side of a handle gives"""
    pos, dirs, _ = default_fan(T)
    g = np.linspace(0.0, 1.0, 41)
    out = {f"coef_{k}": P.coefs(k) for k in FIELDS}
    out["psi_prof_max"] = np.array([T.lib().torj_plasma_psi_prof_max(P.handle)])
    out["volume"] = P.volume(np.linspace(-0.1, 1.3, 29))
    out["shell_volumes"] = P.shell_volumes(g)
    for mode in (1, -1):
        for k, v in zip(("xp", "Np", "s0", "st"), T.ray_entry(P, pos, dirs, OM, mode)):
            out[f"entry{mode}_{k}"] = v
    return out


def assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def AB():
    return tokamak_a(), tokamak_b()


@pytest.fixture(scope="module")
def want(T, AB):
    """fresh handles' host results, computed once"""
    A, B = AB
    return dict(A=host_results(T, fresh(T, A)), B=host_results(T, fresh(T, B)),
                AB=host_results(T, fresh(T, with_profiles(A, B))))


def test_symbols_exported(T):
    L = ctypes.CDLL(T.LIB_PATH)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in T.EXPORTED
    assert T.lib().torj_abi_version() == 8  # symbols added, nothing changed


def test_update_is_a_fresh_create(T, AB, want):
    from torj_hip import synthetic as S

    A, B = AB
    P = fresh(T, A)
    assert_same(host_results(T, P), want["A"])
    P.update(*S.plasma_args(B))
    assert (P.R_coords[0], P.R_coords[-1]) == (1.05, 2.65)
    assert_same(host_results(T, P), want["B"])
    assert not np.array_equal(want["A"]["entry1_xp"], want["B"]["entry1_xp"])  # (the two do differ)
    P.update(*S.plasma_args(A))  # and back
    assert_same(host_results(T, P), want["A"])


def test_update_profiles(T, AB, want):
    A, B = AB
    P = fresh(T, A)
    P.update_profiles(B["psi_prof"], B["ne_prof"], B["Te_prof"])
    got = host_results(T, P)
    assert_same(got, want["AB"])
    for k in ("psi", "Br", "Bz", "Bphi"):  # the equilibrium's slots: bitwise untouched
        assert np.array_equal(got[f"coef_{k}"], want["A"][f"coef_{k}"]), k
    for k in ("lnne", "lnTe"):
        assert not np.array_equal(got[f"coef_{k}"], want["A"][f"coef_{k}"]), k
    # on the equilibrium a full update last gave
    from torj_hip import synthetic as S

    P.update(*S.plasma_args(B))
    P.update_profiles(A["psi_prof"], A["ne_prof"], A["Te_prof"])
    assert_same(host_results(T, P), host_results(T, fresh(T, with_profiles(B, A))))


def coefs_args(T, eq):
    """from_coefs' arguments of the plasma eq: the coefficient arrays a fresh handle built"""
    P = fresh(T, eq)
    c = {k: P.coefs(k) for k in FIELDS}
    n = len(eq["eqt1d_psi_norm"])
    vol = np.linspace(0.0, 17.0, n + 2) ** 1.05
    R, Z = eq["R_coords"], eq["Z_coords"]
    return ((R[0], R[-1]), (Z[0], Z[-1]), c, (eq["eqt1d_psi_norm"][0], eq["eqt1d_psi_norm"][-1]), vol,
            float(eq["psi_prof"].max()))


def test_update_from_coefs(T, AB):
    A, B = AB
    ca, cb = coefs_args(T, A), coefs_args(T, B)
    want_b = host_results(T, T.Plasma.from_coefs(*cb))
    for P in (T.Plasma.from_coefs(*ca), fresh(T, A)):
        P.update_from_coefs(*cb)
        assert_same(host_results(T, P), want_b)
        # no node data now: a profiles-only update is refused, and says why
        with pytest.raises(T.TorjError, match="no psi_norm_data .*coefficients"):
            P.update_profiles(B["psi_prof"], B["ne_prof"], B["Te_prof"])
        assert_same(host_results(T, P), want_b)


def test_profiles_update_of_a_from_coefs_handle_is_refused(T, AB):
    A, B = AB
    P = T.Plasma.from_coefs(*coefs_args(T, A))
    before = host_results(T, P)
    with pytest.raises(T.TorjError) as e:
        P.update_profiles(B["psi_prof"], B["ne_prof"], B["Te_prof"])
    assert str(e.value).startswith("torj_plasma_update_profiles: the handle has no psi_norm_data")
    assert_same(host_results(T, P), before)


def _raw_update(T, h, eq, **kw):
    d = T._lib.dptr
    m = {k: np.ascontiguousarray(np.asarray(eq[k], dtype=np.float64).T)
         for k in ("psi_norm_data", "Br_data", "Bz_data", "Bphi_data")}
    a = dict(p=h, R_coords=d(eq["R_coords"]), Z_coords=d(eq["Z_coords"]), psi_norm_data=d(m["psi_norm_data"]),
             n_prof=len(eq["psi_prof"]), psi_prof=d(eq["psi_prof"]), ne_prof=d(eq["ne_prof"]),
             Te_prof=d(eq["Te_prof"]), Br_data=d(m["Br_data"]), Bz_data=d(m["Bz_data"]),
             Bphi_data=d(m["Bphi_data"]), n_eq=len(eq["eqt1d_psi_norm"]), eqt1d_psi_norm=d(eq["eqt1d_psi_norm"]),
             eqt1d_volume=d(eq["eqt1d_volume"]))
    a.update(kw)
    rc = T.lib().torj_plasma_update(*a.values(), None)
    return rc, T.lib().torj_last_error().decode()


def _raw_coefs(T, h, args, **kw):
    d = T._lib.dptr
    (R1, Rn), (Z1, Zn), c, (v1, vn), vol, pmax = args
    ct = {k: np.ascontiguousarray(c[k].T) for k in FIELDS}
    a = dict(p=h, R1=R1, Rn=Rn, Z1=Z1, Zn=Zn, coef_psi=d(ct["psi"]), coef_lnne=d(ct["lnne"]), coef_lnTe=d(ct["lnTe"]),
             coef_Br=d(ct["Br"]), coef_Bz=d(ct["Bz"]), coef_Bphi=d(ct["Bphi"]), n_vol=len(vol) - 2, vol_psi1=v1,
             vol_psin=vn, vol_coefs=d(vol), psi_prof_max=pmax)
    a.update(kw)
    rc = T.lib().torj_plasma_update_from_coefs(*a.values(), None)
    return rc, T.lib().torj_last_error().decode()


def _raw_profiles(T, h, eq, **kw):
    d = T._lib.dptr
    a = dict(p=h, n_prof=len(eq["psi_prof"]), psi_prof=d(eq["psi_prof"]), ne_prof=d(eq["ne_prof"]),
             Te_prof=d(eq["Te_prof"]))
    a.update(kw)
    rc = T.lib().torj_plasma_update_profiles(*a.values(), None)
    return rc, T.lib().torj_last_error().decode()


def test_refusals_name_the_argument_and_leave_the_handle(T, AB, want):
    A, B = AB
    P = fresh(T, A)
    h = P.handle
    cb = coefs_args(T, B)
    cases = []
    # torj_plasma_update
    cases.append((_raw_update(T, None, B), "torj_plasma_update: p is NULL"))
    for name in ("R_coords", "Z_coords", "psi_norm_data", "psi_prof", "ne_prof", "Te_prof", "Br_data", "Bz_data",
                 "Bphi_data", "eqt1d_psi_norm", "eqt1d_volume"):
        cases.append((_raw_update(T, h, B, **{name: None}), f"torj_plasma_update: {name} is NULL"))
    cases.append((_raw_update(T, h, B, n_prof=1), "torj_plasma_update: n_prof = 1 < 2"))
    cases.append((_raw_update(T, h, B, n_eq=0), "torj_plasma_update: n_eq = 0 < 2"))
    # torj_plasma_update_from_coefs
    cases.append((_raw_coefs(T, None, cb), "torj_plasma_update_from_coefs: p is NULL"))
    for name in ("coef_psi", "coef_lnne", "coef_lnTe", "coef_Br", "coef_Bz", "coef_Bphi", "vol_coefs"):
        cases.append((_raw_coefs(T, h, cb, **{name: None}), f"torj_plasma_update_from_coefs: {name} is NULL"))
    cases.append((_raw_coefs(T, h, cb, n_vol=1), "torj_plasma_update_from_coefs: n_vol = 1 < 2"))
    # torj_plasma_update_profiles
    cases.append((_raw_profiles(T, None, B), "torj_plasma_update_profiles: p is NULL"))
    for name in ("psi_prof", "ne_prof", "Te_prof"):
        cases.append((_raw_profiles(T, h, B, **{name: None}), f"torj_plasma_update_profiles: {name} is NULL"))
    cases.append((_raw_profiles(T, h, B, n_prof=-3), "torj_plasma_update_profiles: n_prof = -3 < 2"))
    for (rc, msg), text in cases:
        assert rc != 0 and msg == text, (msg, text)
    assert_same(host_results(T, P), want["A"])
    # the cell table: only once the device state exists
    out = np.zeros((NZ - 1, NR - 1, 96))
    assert T.lib().torj_plasma_get_cell_table(None, T._lib.dptr(out)) != 0
    assert T.lib().torj_last_error().decode() == "torj_plasma_get_cell_table: p is NULL"
    assert T.lib().torj_plasma_get_cell_table(h, None) != 0
    assert T.lib().torj_last_error().decode() == "torj_plasma_get_cell_table: out is NULL"
    # the valid calls go through on the same handle afterwards
    assert _raw_update(T, h, B)[0] == 0
    assert_same(host_results(T, P), want["B"])


def test_wrapper_keeps_the_grid_size(T, AB):
    from torj_hip import synthetic as S

    P = fresh(T, AB[0])
    with pytest.raises(ValueError, match="grid size"):
        P.update(*S.plasma_args(S.circular_tokamak(nR=NR + 1, nZ=NZ)))


def test_cell_table_needs_the_device_state(T, AB):
    """before the handle's first GPU use there is no table to read"""
    P = fresh(T, AB[0])
    with pytest.raises(T.TorjError, match="no device state yet"):
        P.cell_table()
