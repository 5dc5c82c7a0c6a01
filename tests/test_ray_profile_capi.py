"""torj_ray_profile[_device] at the C-ABI boundary (include/torj_hip.h), without a GPU:
the symbols are exported, every refusal comes back by its exact text through the raw C
call on handles never used on the GPU (all arguments are checked before any HIP call),
and the header's TORJ_PROF_* enum is the mirror's column order.

Also here, with the oracle alone: the preconditions of the GPU scenario of
tests/test_gpu_ray_profile.py, whose workload (BEAMS, workload()) lives here -- among
its 32 rays at 12 000 steps with checks every 120 one ends OK, one LEFT_PLASMA and one
ABSORBED, and one stops at a step count that is no multiple of the row stride, so that
a partly NaN table and a cut between two rows are both exercised."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

DS, N_STEPS, CHUNK, STRIDE = 1e-4, 12000, 120, 1000
N_ROWS = N_STEPS // STRIDE + 1
# frequency, mode, steering pol / tor (degrees), rays taken from the default 46-ray fan
BEAMS = (
    (92.5e9, 1, 30.0, 0.0, 13),
    (92.5e9, -1, 30.0, 0.0, 5),
    (140e9, 1, 30.0, 0.0, 0),
    (110e9, 1, 30.0, 0.0, 1),
    (85.5e9, -1, 25.0, 5.0, 13),
)
OFF = [0, 13, 18, 18, 19, 32]


def workload(T, plasma):
    """The five beams' concatenated entry states (host ray entry) and their tables."""
    from torj_hip import synthetic as S

    s = S.SETUP
    xp, Np, s0, off, omega, mode = [], [], [], [0], [], []
    for f, m, pol, tor, k in BEAMS:
        N0 = T.pol_tor_angles_2_vector(np.deg2rad(pol), np.deg2rad(tor))
        pos, dirs, w = T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"],
                                                s["inverse_curvature_radius"], f)
        assert len(w) == 46
        om = 2 * np.pi * f
        x, N, sv, st = T.ray_entry(plasma, pos, dirs, om, m)
        assert (st == 0).all()
        xp.append(x[:k]), Np.append(N[:k]), s0.append(sv[:k])
        off.append(off[-1] + k), omega.append(om), mode.append(m)
    assert off == OFF
    return dict(off=off, omega=omega, mode=mode, xp=np.concatenate(xp), Np=np.concatenate(Np),
                s0=np.concatenate(s0))


def oracle_beams(oplasma, b, n_steps=N_STEPS, **kw):
    """the oracle's trace of every non-empty beam with its own frequency and mode -> {beam: result}"""
    out = {}
    for k in range(len(b["omega"])):
        sl = slice(b["off"][k], b["off"][k + 1])
        if sl.start < sl.stop:
            out[k] = oplasma.trace(b["xp"][sl], b["Np"][sl], b["omega"][k], b["mode"][k], DS, n_steps,
                                   chunk_steps=CHUNK, **kw)
    return out


@pytest.fixture(scope="module")
def plasma(T):
    """a handle of its own, never used on a GPU"""
    from torj_hip import synthetic as S

    return T.Plasma(*S.plasma_args(S.circular_tokamak()))


def test_symbols_exported(T):
    L = C.CDLL(T.LIB_PATH)
    for sym in ("torj_ray_profile", "torj_ray_profile_device"):
        assert hasattr(L, sym)
        assert sym in T.EXPORTED
    assert T.lib().torj_abi_version() == 8  # symbols added, nothing changed


def test_enum_order_is_the_mirrors_columns(T):
    """TORJ_PROF_<NAME> in the header's order against RayProfile.columns; the header
    spells the plasma's X and Y X_PL and Y_PL (X and Y are the point's coordinates)"""
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "torj_hip.h")).read(), flags=re.S)
    body = re.search(r"enum\s*\{([^}]*TORJ_PROF_NCOL[^}]*)\}", h).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert names[-1] == "TORJ_PROF_NCOL" and len(names) == 26
    assert "TORJ_PROF_X = 0" in body
    want = {"X_PL": "X", "Y_PL": "Y", "X": "x", "Y": "y", "Z": "z", "NX": "Nx", "NY": "Ny", "NZ": "Nz",
            "TAU": "tau", "S": "s", "P": "P", "ALPHA": "alpha", "DP_DS": "dP_ds", "PSI": "psi", "NE": "ne",
            "TE": "Te", "BX": "Bx", "BY": "By", "BZ": "Bz", "B_ABS": "B_abs", "N_PAR": "N_par",
            "N_ABS": "N_abs", "NS2": "Ns2", "LAMBDA": "Lambda", "DLAMBDA_DN": "dLambda_dN"}
    got = tuple(want[n[len("TORJ_PROF_"):]] for n in names[:-1])
    assert got == T.RayProfile.columns == T.PROFILE_COLUMNS
    assert len(set(got)) == 25


def raw(T, p, device=False, **kw):
    """torj_ray_profile[_device] called directly on one 3-ray beam -> (rc, error text)"""
    from torj_hip._lib import TraceCfg, dptr, handles, iptr

    n = 3
    a = dict(p=p.handle if p is not None else None, n_plasmas=0, plasmas=None, beam_plasma=None,
             cfg=TraceCfg(0.0, 0, 1e-4, 100, 10, 1.0, 1e-6, 1, 10), n_beams=1,
             off=np.array([0, n], dtype=np.int32), omega=np.array([2 * np.pi * 92.5e9]),
             mode=np.array([1], dtype=np.int32), x0=np.ones((3, n)), N0=np.ones((3, n)), s0=None, n_rows=11,
             prof=np.zeros((11, 25, n)), state=np.zeros((7, n)), status=np.zeros(n, dtype=np.int32),
             steps=np.zeros(n, dtype=np.int32))
    a.update(kw)
    pl, bp = a["plasmas"], a["beam_plasma"]
    head = (a["p"], a["n_plasmas"], handles(pl) if pl is not None else None,
            iptr(np.ascontiguousarray(bp, dtype=np.int32)) if bp is not None else None, a["cfg"], a["n_beams"],
            iptr(a["off"]), dptr(a["omega"]), iptr(a["mode"]))
    if device:  # never reaches the device: the pointers only have to be non-NULL where an array stands
        vp = lambda v: v.ctypes.data if v is not None else None
        rc = T.lib().torj_ray_profile_device(*head, vp(a["x0"]), vp(a["N0"]), vp(a["s0"]), a["n_rows"], vp(a["prof"]),
                                             vp(a["state"]), vp(a["status"]), vp(a["steps"]), None)
    else:
        rc = T.lib().torj_ray_profile(*head, dptr(a["x0"]), dptr(a["N0"]), dptr(a["s0"]), a["n_rows"],
                                      dptr(a["prof"]), dptr(a["state"]), iptr(a["status"]), iptr(a["steps"]))
    return rc, T.lib().torj_last_error().decode()


def err(T, p, **kw):
    rc, text = raw(T, p, **kw)
    assert rc != 0
    return text


def cfg(T, **kw):
    from torj_hip._lib import TraceCfg

    a = dict(omega=0.0, mode=0, ds=1e-4, n_steps=100, chunk_steps=10, psi_exit=1.0, P_min=1e-6, absorption=1,
             traj_stride=10, deposition=0, integrator=0)
    a.update(kw)
    return TraceCfg(**a)


@pytest.mark.parametrize("device", [False, True])
def test_own_refusals(T, plasma, device):
    p = plasma
    assert err(T, p, device=device, prof=None) == "torj_ray_profile: prof is NULL"
    for stride in (0, -2):
        assert err(T, p, device=device, cfg=cfg(T, traj_stride=stride)) == \
            f"torj_ray_profile: traj_stride = {stride} < 1"
    for n_steps in (0, -1):
        assert err(T, p, device=device, cfg=cfg(T, n_steps=n_steps)) == f"torj_ray_profile: n_steps = {n_steps} < 1"
    for n_rows in (10, 12, 0):
        assert err(T, p, device=device, n_rows=n_rows) == \
            f"torj_ray_profile: n_rows = {n_rows}, but n_steps / traj_stride + 1 = 11"
    # n_steps / traj_stride is the integer quotient: 105 steps, stride 10 -> 11 rows
    assert err(T, p, device=device, cfg=cfg(T, n_steps=105), n_rows=12) == \
        "torj_ray_profile: n_rows = 12, but n_steps / traj_stride + 1 = 11"
    assert err(T, None, device=device) == "torj_ray_profile: p is NULL"
    assert err(T, p, device=device, cfg=None) == "torj_ray_profile: cfg is NULL"


@pytest.mark.parametrize("device", [False, True])
def test_multi_beam_refusals_come_through(T, plasma, device):
    """beams_plan's and beams_plasmas_check's refusals by their existing texts"""
    p = plasma
    for model in (2, 3):
        assert err(T, p, device=device, cfg=cfg(T, absorption=model)) == \
            "absorption must be 0 or 1 in a multi-beam launch (the warm models trace one beam per call)"
    assert err(T, p, device=device, cfg=cfg(T, integrator=1)) == \
        "integrator must be 0 in a multi-beam launch (the adaptive integrator traces one beam per call)"
    try:
        for sched in (3, 1):
            p.set_sched(sched)
            assert err(T, p, device=device) == \
                f"sched mode {sched} has no multi-beam form: only the one-shot kernel (torj_set_sched -1, 0, 2)"
    finally:
        p.set_sched(-1)
    assert err(T, p, device=device, off=np.array([1, 3], dtype=np.int32)) == "beam_off[0] must be 0"
    assert err(T, p, device=device, n_beams=2, off=np.array([0, 3, 2], dtype=np.int32), omega=np.full(2, 6e11),
               mode=np.array([1, -1], dtype=np.int32)) == "beam_off must not decrease (beam 1)"
    assert err(T, p, device=device, n_beams=0) == "n_beams must be 1..4096"
    assert err(T, p, device=device, mode=np.array([0], dtype=np.int32)) == "mode[0] must be +1 (X) or -1 (O)"
    assert err(T, p, device=device, x0=None) == "x0, N0, state, status, steps required"
    # the plasma tables: both or neither, indices in range
    assert err(T, p, device=device, n_plasmas=1, plasmas=None) == "plasmas is NULL"
    assert err(T, p, device=device, n_plasmas=0, plasmas=[p], beam_plasma=[0]) == "n_plasmas must be 1..4096"
    assert err(T, p, device=device, n_plasmas=1, plasmas=[p], beam_plasma=None) == "beam_plasma is NULL"
    assert err(T, p, device=device, n_plasmas=1, plasmas=[p], beam_plasma=[1]) == \
        "beam_plasma[0] = 1 is outside 0..0 (n_plasmas = 1)"
    # deposition is not read
    rc, text = raw(T, p, device=device, cfg=cfg(T, deposition=7), prof=None)
    assert rc != 0 and text == "torj_ray_profile: prof is NULL"


def test_mirror_refuses_before_any_device_work(T, plasma):
    b = dict(off=[0, 2], omega=[6e11], mode=[1], xp=np.ones((2, 3)), Np=np.ones((2, 3)))
    with pytest.raises(T.TorjError, match=r"torj_ray_profile: traj_stride = 0 < 1"):
        T.ray_profile(plasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], n_steps=100, traj_stride=0)
    with pytest.raises(T.TorjError, match="warm models trace one beam per call"):
        T.ray_profile(plasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], n_steps=100, traj_stride=10,
                      absorption="warm_wr")
    with pytest.raises(ValueError, match="beam_off"):
        T.ray_profile(plasma, [0, 3], b["omega"], b["mode"], b["xp"], b["Np"], n_steps=100, traj_stride=10)


def test_gpu_scenario_preconditions(T, plasma, oplasma):
    """The oracle alone on the GPU scenario's rays: all three endings, a stop between two rows."""
    b = workload(T, plasma)
    assert T.ray_profile is not None  # (the scenario is this call's)
    res = oracle_beams(oplasma, b)
    status = np.concatenate([res[k]["status"] for k in sorted(res)])
    steps = np.concatenate([res[k]["steps"] for k in sorted(res)])
    assert len(status) == 32
    print("status", status.tolist())
    print("steps", steps.tolist())
    assert {T.OK, T.LEFT_PLASMA, T.ABSORBED} <= set(status.tolist())
    assert (steps[status == T.OK] == N_STEPS).all()
    assert (steps % STRIDE != 0).any()
    assert (steps % CHUNK == 0).all()
    # the X-mode beam is absorbed on its way (the dP/ds check there is not one of zeros)
    assert res[0]["state"][:, 6].min() > 1.0
