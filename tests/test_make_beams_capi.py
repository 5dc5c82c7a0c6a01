"""torj_make_beams at the C-ABI boundary (include/torj_hip.h), without a GPU: the
symbol is exported, every refusal comes back by its exact text through the raw C
call on handles never used on the GPU (all arguments are checked before any HIP
call), and the count-only call gives torj_launch_peripheral_rays' counts.

Also here, on the host ray entry: the preconditions of the GPU scenarios of
tests/test_gpu_make_beams.py -- a launcher whose fan enters the plasma in part
(GRAZING) and one none of whose rays enter (MISSING)."""
import ctypes as C

import numpy as np
import pytest

F0 = 92.5e9
GRID = np.linspace(0.0, 1.0, 200)


def launcher(pol_deg, tor_deg=0.0, f=F0, mode=1):
    """make_beam's leading arguments at SETUP's launch point"""
    from torj_hip import synthetic as S

    s = S.SETUP
    return (s["R0"], s["phi0"], s["z0"], np.deg2rad(tor_deg), np.deg2rad(pol_deg), s["spot_size"],
            s["inverse_curvature_radius"], f, mode)


# SETUP's launch point, 92.5 GHz, X-mode, tor 0: the poloidal angle scanned upward from 30
# degrees in 0.5 degree steps on the CPU (host ray entry, circular_tokamak()): all 46 rays
# enter up to 63.0, then 41, 39, 36, 32 (65.0), 30, 23, 19, 15, 11, 7, 5, 1 (69.0), and none
# from 69.5 on
GRAZING_POL, GRAZING_OK, GRAZING_FIRST_BAD = 65.0, 32, (5, 5)  # (ray within the beam, ENTRY_FAIL)
MISSING_POL = 75.0


@pytest.fixture(scope="module")
def plasma(T):
    from torj_hip import synthetic as S

    return T.Plasma(*S.plasma_args(S.circular_tokamak()))


def host_entry(T, plasma, la):
    """the launcher's fan and its host ray entry -> (pos, dirs, w, xp, Np, s0, status)"""
    r, phi, z, tor, pol, spot, inv_curv, f, mode = la
    N0 = T.pol_tor_angles_2_vector(pol, tor)
    fan = T.launch_peripheral_rays([r * np.cos(phi), r * np.sin(phi), z], N0, spot, inv_curv, f)
    return (*fan, *T.ray_entry(plasma, fan[0], fan[1], 2.0 * np.pi * f, mode))


def test_symbol_exported(T):
    L = C.CDLL(T.LIB_PATH)
    assert hasattr(L, "torj_make_beams")
    assert "torj_make_beams" in T.EXPORTED
    assert T.lib().torj_abi_version() == 8  # a symbol added, nothing changed


def test_structs_match_the_header():
    """the mirror's three ctypes structs against the C structs' sizes as the header lays them out"""
    from torj_hip._lib import BeamResult, BeamsRays, Launcher

    assert C.sizeof(Launcher) == 8 * 8 + 2 * 4
    assert C.sizeof(BeamResult) == 4 * 4 + 2 * 8
    assert C.sizeof(BeamsRays) == 12 * C.sizeof(C.c_void_p)
    assert [n for n, _ in Launcher._fields_] == ["r", "phi", "z", "steering_angle_tor", "steering_angle_pol",
                                                 "spot_size", "inverse_curvature_radius", "f", "mode", "plasma"]


def test_grazing_launcher_enters_in_part(T, plasma):
    st = host_entry(T, plasma, launcher(GRAZING_POL))[6]
    assert len(st) == 46
    n_ok = int((st == 0).sum())
    assert 5 <= n_ok <= 41
    assert n_ok == GRAZING_OK
    bad = np.flatnonzero(st != 0)
    assert (int(bad[0]), int(st[bad[0]])) == GRAZING_FIRST_BAD


def test_missing_launcher_enters_nothing(T, plasma):
    st = host_entry(T, plasma, launcher(MISSING_POL))[6]
    assert len(st) == 46 and int((st == 0).sum()) == 0


def raw(T, p, launchers=(launcher(30.0),), **kw):
    """torj_make_beams called directly -> (rc, error text, ray_off); keywords replace arguments"""
    from torj_hip._lib import BeamResult, BeamsRays, Launcher, TraceCfg, dptr, handles, iptr

    B = len(launchers) if launchers is not None else 1
    la = None
    if launchers is not None:
        la = (Launcher * B)(*[Launcher(*map(float, l[:8]), int(l[8]), int(l[9]) if len(l) > 9 else 0)
                              for l in launchers])
    a = dict(p=p.handle if p is not None else None, n_plasmas=0, plasmas=None, n_beams=B, launchers=la, N_rings=3,
             min_az=5, cfg=TraceCfg(0.0, 0, 1e-4, 100, 1, 1.0, 1e-6, 1, 1, 1), n_psi=len(GRID), grid=GRID,
             dP_dV=np.zeros((max(B, 1), len(GRID))), res=(BeamResult * max(B, 1))(),
             off=np.full(max(B, 1) + 1, -1, dtype=np.int32), rays=BeamsRays())
    a.update(kw)
    pl = a["plasmas"]
    rc = T.lib().torj_make_beams(a["p"], a["n_plasmas"], handles(pl) if pl is not None else None, a["n_beams"],
                                 a["launchers"], a["N_rings"], a["min_az"], a["cfg"], a["n_psi"], dptr(a["grid"]),
                                 dptr(a["dP_dV"]), a["res"], iptr(a["off"]), a["rays"])
    return rc, T.lib().torj_last_error().decode(), a["off"]


def err(T, p, *args, **kw):
    rc, text, _ = raw(T, p, *args, **kw)
    assert rc != 0
    return text


def test_rejections(T, plasma):
    p = plasma
    assert err(T, p, launchers=None) == "torj_make_beams: launchers is NULL"
    assert err(T, p, cfg=None) == "torj_make_beams: cfg is NULL"
    assert err(T, p, grid=None) == "torj_make_beams: psi_dP_dV is NULL"
    assert err(T, None) == "torj_make_beams: p is NULL"
    assert err(T, p, n_beams=0) == "torj_make_beams: n_beams must be 1..4096"
    assert err(T, p, n_beams=-1) == "torj_make_beams: n_beams must be 1..4096"
    assert err(T, p, n_beams=4097) == "torj_make_beams: n_beams must be 1..4096"
    for n_psi in (1, 0, -3):
        assert err(T, p, n_psi=n_psi) == "torj_make_beams: n_psi must be >= 2"
    good = launcher(30.0)
    for bad in (0.0, -F0, float("nan"), float("inf")):
        assert err(T, p, [good, launcher(30.0, f=bad)]) == "torj_make_beams: launchers[1].f must be finite and > 0"
    for bad in (0, 2, -2):
        assert err(T, p, [good, good, launcher(30.0, mode=bad)]) == \
            "torj_make_beams: launchers[2].mode must be +1 (X) or -1 (O)"
    assert err(T, p, N_rings=1) == "ArgumentError: N_rings = 1 < 2 which is the minimum"


def test_plasma_table_rejections(T, plasma):
    from torj_hip import synthetic as S

    p = plasma
    q = T.Plasma(*S.plasma_args(S.circular_tokamak(Te0=6000, ne_scale=0.6)))
    far = T.Plasma(*S.plasma_args(S.circular_tokamak()), device=1)
    good = launcher(30.0)
    both = "torj_make_beams: n_plasmas = %d with plasmas %s (n_plasmas == 0 and plasmas == NULL: every beam " \
           "through p; else n_plasmas >= 1 listed handles)"
    assert err(T, p, n_plasmas=2) == both % (2, "NULL")
    assert err(T, p, n_plasmas=0, plasmas=[p, q]) == both % (0, "given")
    assert err(T, p, n_plasmas=-1, plasmas=[p, q]) == both % (-1, "given")
    for bad in (-1, 2):
        assert err(T, p, [good + (1,), good + (bad,)], n_plasmas=2, plasmas=[p, q]) == \
            f"torj_make_beams: launchers[1].plasma = {bad} is outside 0..1 (n_plasmas = 2)"
    # the rules of torj_trace_beams_plasmas, by its texts
    assert err(T, p, [good + (0,)], n_plasmas=2, plasmas=[p, None]) == "plasmas[1] is NULL"
    assert err(T, p, [good + (0,)], n_plasmas=2, plasmas=[p, far]) == \
        "plasmas[1] is on device 1, the launching handle on device 0 (one device per launch)"
    assert err(T, p, [good + (0,)], n_plasmas=4097, plasmas=[p] * 4097) == "n_plasmas must be 1..4096"


def test_trace_refusals_come_through(T, plasma):
    """torj_trace_beams' refusals by their existing texts, before any device work"""
    from torj_hip._lib import TraceCfg

    p = plasma
    for a in (2, 3):
        assert err(T, p, cfg=TraceCfg(0.0, 0, 1e-4, 100, 1, 1.0, 1e-6, a, 1, 1)) == \
            "absorption must be 0 or 1 in a multi-beam launch (the warm models trace one beam per call)"
    assert err(T, p, cfg=TraceCfg(0.0, 0, 1e-4, 100, 1, 1.0, 1e-6, 1, 1, 1, 1, s_max=0.01)) == \
        "integrator must be 0 in a multi-beam launch (the adaptive integrator traces one beam per call)"
    assert err(T, p, cfg=TraceCfg(0.0, 0, 0.0, 100, 1, 1.0, 1e-6, 1, 1, 1)) == "ds must be > 0"
    try:
        for m in (1, 3):
            p.set_sched(m)
            assert err(T, p) == \
                f"sched mode {m} has no multi-beam form: only the one-shot kernel (torj_set_sched -1, 0, 2)"
    finally:
        p.set_sched(-1)
    grid = GRID.copy()
    grid[7] = grid[6]
    assert err(T, p, grid=grid) == "psi_dP_dV must be strictly increasing"


@pytest.mark.parametrize("N_rings", [2, 3, 5])
def test_count_only(T, plasma, N_rings):
    """dP_dV, res and rays NULL, ray_off given: the launched offsets, each launcher's count
    torj_launch_peripheral_rays' own (its two-call pattern); nothing else is read, so the
    call needs no plasma, cfg or grid"""
    las = [launcher(30.0), launcher(35.0, -5.0, 100e9), launcher(25.0, 5.0, 85.5e9, -1),
           (*launcher(30.0)[:5], 0.03, 1.0 / 2.5, 140e9, 1)]
    for min_az in (5, 7):
        want = [0]
        for r, phi, z, tor, pol, spot, inv_curv, f, mode in las:
            n = C.c_int(-1)
            x0 = np.array([r * np.cos(phi), r * np.sin(phi), z])
            N0 = T.pol_tor_angles_2_vector(pol, tor)
            assert T.lib().torj_launch_peripheral_rays(T._lib.dptr(x0), T._lib.dptr(N0), spot, inv_curv, f, N_rings,
                                                       min_az, 1, C.byref(n), None, None, None) == 0
            want.append(want[-1] + n.value)
        for p, kw in ((plasma, {}), (None, dict(cfg=None, grid=None, n_psi=0))):
            rc, text, off = raw(T, p, las, N_rings=N_rings, min_az=min_az, dP_dV=None, res=None, rays=None, **kw)
            assert rc == 0, text
            assert list(off) == want
        assert want[4] > 4 * N_rings  # more than one ray per ring
    # the count-only call refuses what it reads
    assert err(T, plasma, las, N_rings=1, dP_dV=None, res=None, rays=None) == \
        "ArgumentError: N_rings = 1 < 2 which is the minimum"
    assert err(T, plasma, las, n_beams=0, dP_dV=None, res=None, rays=None) == "torj_make_beams: n_beams must be 1..4096"


def test_wrapper_wants_both_tables(T, plasma):
    with pytest.raises(ValueError, match="go together"):
        T.make_beams_c(plasma, [launcher(30.0)], 0.01, GRID, plasmas=[plasma])
    with pytest.raises(ValueError, match="n_beams entries"):
        T.make_beams_c(plasma, [launcher(30.0)], 0.01, GRID, plasmas=[plasma], beam_plasma=[0, 0])
    with pytest.raises(ValueError, match="N_rings = 1 < 2"):
        T.make_beams_c(plasma, [launcher(30.0)], 0.01, GRID, N_rings=1)
