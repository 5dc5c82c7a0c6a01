"""Warm-absorption trace scenarios off the one X2 fan (helper module of
tests/test_warm_cases.py and tests/test_gpu_warm_paths.py; generated, no fixture).

Every other warm trace in the suite is SETUP's perpendicular fan (|N_par| <~ 0.01)
at 92.5 GHz, X-mode, through circular_tokamak().  The scenarios here leave it:

  A  x2_oblique      circular_tokamak(), 92.5 GHz, tor 20 deg, X and O: N_par 0.37 - 0.43
  B  o1_fundamental  circular_tokamak(ne0=1.5e19), 60 GHz, tor 10 deg, O: Y crosses 1
  C  shaped_lfs_down shaped_eq, either field direction, LAUNCHES["lfs_down"] rotated by
                     PHI_ROT, 92.5 GHz, X and O: N_par -0.22 .. -0.32
  D  hot_x3_oblique  circular_tokamak(Te0=25e3), 140 GHz, tor 20 deg, X and O: Larmor
                     order 4 or the cap 5 at every point, so every point is deferred
  E  x3_mixed        circular_tokamak(), 140 GHz, tor 0, X: Larmor orders 3 and 4 mixed,
                     so waves are partly deferred
  F  hot_stops       D's plasma, 140 GHz, tor 0, X: a 66-ray fan ABSORBED at differing
                     steps plus two outward rays that end LEFT_PLASMA (68 rays: two
                     groups, the last one partial)

A to E launch launch_peripheral_rays(N_rings=2, min_azimuthal_points=3), 12 rays, from
SETUP's point with pol 30 deg; every trace takes steps of 1e-3 m.  The entry states are
the oracle's, and the oracle's traces are kept per (scenario, mode, model, variant) for
the tests that share them.  The tau ranges are the C oracle's own figures for model 2
and 3 alike (tests/test_warm_cases.py holds the oracle to them, widened by 10 %)."""
import numpy as np

import shaped_eq as E
from torj_hip import synthetic as S

DS = 1e-3
STRIDE = 10  # trajectory samples every 10 steps
OK, LEFT_PLASMA, ABSORBED = 0, 1, 2
BAR_TAU = {2: 1e-8, 3: 1e-9}  # the project's warm tau bars (tests/test_gpu_warm.py)
TAU_FLOOR, ETA = 1e-6, 2.0 ** -45  # tests/test_gpu_c5.py
IWARM = {2: 1, 3: 3}

PLASMAS = {
    "circ": lambda: S.plasma_args(S.circular_tokamak()),
    "ne15": lambda: S.plasma_args(S.circular_tokamak(ne0=1.5e19)),
    "hot": lambda: S.plasma_args(S.circular_tokamak(Te0=25e3)),
    "s+": lambda: E.shaped_args(sigma=1.0),
    "s-": lambda: E.shaped_args(sigma=-1.0),
}

# name -> plasma, frequency, toroidal steering in degrees, modes, steps, oracle's tau range per mode
SCENARIOS = {
    "A": dict(name="x2_oblique", plasma="circ", f=92.5e9, tor=20.0, modes=(1, -1), n_steps=400,
              tau={1: (8.9, 10.2), -1: (0.157, 0.186)}),
    "B": dict(name="o1_fundamental", plasma="ne15", f=60e9, tor=10.0, modes=(-1,), n_steps=1000,
              tau={-1: (13.8, 14.9)}, tau_no_stop={-1: (16.5, 18.4)}),
    "C": dict(name="shaped_lfs_down", plasma="s+", f=E.F, tor=None, modes=(1, -1), n_steps=600,
              tau={1: (11.5, 13.5), -1: (0.229, 0.267)}),
    "D": dict(name="hot_x3_oblique", plasma="hot", f=140e9, tor=20.0, modes=(1, -1), n_steps=600,
              tau={1: (7.7, 9.2), -1: (0.38, 0.49)}),
    "E": dict(name="x3_mixed", plasma="circ", f=140e9, tor=0.0, modes=(1,), n_steps=600,
              tau={1: (0.063, 0.089)}),
    "F": dict(name="hot_stops", plasma="hot", f=140e9, tor=0.0, modes=(1,), n_steps=600, tau=None),
}
# (scenario, mode) pairs and their test ids
PAIRS = [(k, m) for k in "ABCDE" for m in SCENARIOS[k]["modes"]]
PAIR_IDS = [f"{k}-{'X' if m == 1 else 'O'}" for k, m in PAIRS]
F_RINGS, F_MIN_AZ = 4, 4  # F's fan: 66 rays
# ABSORBED steps of F's fan in the oracle, per model
F_STOPS = {2: (570, 588), 3: (516, 534)}

# the adaptive integrator's power clamp fed by a warm alpha: B with dtmax 2 cm and loose
# tolerances, 1 m in 20 chunks (alpha ds up to 3.5: Tsit5's steps overshoot P below zero)
CLAMP = dict(ds=2e-2, s_max=1.0, n_chunks=20, abstol=1.0, reltol=1.0, integrator=1, s0="entry", traj_stride=1)
CLAMP_CAP = 400

_plasmas, _rays, _runs = {}, {}, {}


def omega(key):
    return 2.0 * np.pi * SCENARIOS[key]["f"]


def oracle_plasma(O, pk):
    if pk not in _plasmas:
        _plasmas[pk] = O.OraclePlasma(*PLASMAS[pk]())
    return _plasmas[pk]


def launch(M, key):
    """launch_peripheral_rays of module M (torj_hip or the oracle) for a scenario:
    (pos, dirs, weights); F without its two outward rays"""
    sc, s = SCENARIOS[key], S.SETUP
    rings, az = (F_RINGS, F_MIN_AZ) if key == "F" else (2, 3)
    if key == "C":
        return E.fan(M, E.LAUNCHES["lfs_down"], rings, az, E.PHI_ROT, sc["f"])
    N0 = M.pol_tor_angles_2_vector(s["steering_angle_pol"], np.deg2rad(sc["tor"]))
    return M.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"], s["inverse_curvature_radius"],
                                    sc["f"], N_rings=rings, min_azimuthal_points=az)


def outward_rays(op, om):
    """test_split_termination_vs_oracle's two rays launched outwards from inside the
    plasma, |N| put on the X-mode dispersion surface by the same bisection"""
    x = np.array([[2.1, 0.0, 0.0], [1.9, 0.0, 0.3]])
    N = np.array([[1.0, 0.0, 0.0], [0.2, 0.0, 1.0]])
    for i in range(len(x)):
        N[i] /= np.linalg.norm(N[i])
        lo, hi = 0.01, 1.5
        for _ in range(100):
            m = 0.5 * (lo + hi)
            d = op.dispersion_relation(x[i], N[i] * m, om, 1)
            lo, hi = (m, hi) if d < 0 else (lo, m)
        N[i] *= lo
    return x, N


def rays(O, key, mode, pk=None):
    """One scenario's launch and its entry into the scenario's plasma (pk: another plasma,
    C's reversed field) by the oracle, every ray entering with status 0: dict of pos, dirs,
    w, xp, Np, s0, n_fan (the rays that came through the entry; F appends two that start
    inside, with the launch point standing in for pos and s0 = 0)"""
    pk = pk or SCENARIOS[key]["plasma"]
    if (key, mode, pk) not in _rays:
        from test_oracle_symmetry import oracle_entry

        op, om = oracle_plasma(O, pk), omega(key)
        pos, dirs, w = launch(O, key)
        st, xp, Np, s0 = oracle_entry(op, pos, dirs, mode, om)
        assert (st == 0).all(), (key, mode, pk, st)
        n_fan = len(w)
        if key == "F":
            xo, No = outward_rays(op, om)
            pos, dirs = np.vstack([pos, xo]), np.vstack([dirs, No / np.linalg.norm(No, axis=1)[:, None]])
            xp, Np, s0 = np.vstack([xp, xo]), np.vstack([Np, No]), np.concatenate([s0, [0.0, 0.0]])
            w = np.concatenate([w, [w.min(), w.min()]])
        _rays[key, mode, pk] = dict(pos=pos, dirs=dirs, w=w, xp=xp, Np=Np, s0=s0, n_fan=n_fan, pk=pk)
    return _rays[key, mode, pk]


def oracle_trace(O, key, mode, model, pk=None, n_steps=None, **kw):
    """The C oracle's trace of a scenario (kept): steps of DS, the scenario's step count
    unless n_steps says otherwise, samples every STRIDE steps, further oracle.trace
    keywords in kw (hashable values; psi_grid=n stands for linspace(0, 1, n) with the
    rays' weights, s0="entry" for the entry's path lengths, ds for another step than DS)"""
    r = rays(O, key, mode, pk)
    n_steps = n_steps or SCENARIOS[key]["n_steps"]
    k = (key, mode, model, r["pk"], n_steps, tuple(sorted(kw.items())))
    if k not in _runs:
        kw = dict(kw)
        if "psi_grid" in kw:
            kw.update(psi_grid=np.linspace(0.0, 1.0, kw["psi_grid"]), weights=r["w"])
        if kw.get("s0") == "entry":
            kw["s0"] = r["s0"]
        kw.setdefault("traj_stride", STRIDE)
        _runs[k] = oracle_plasma(O, r["pk"]).trace(r["xp"], r["Np"], omega(key), mode, kw.pop("ds", DS), n_steps,
                                                   absorption=model, **kw)
    return _runs[k]


def flagged(O, key, mode, model, o, pk=None):
    """tests/test_gpu_c5.py's a-priori conditioning flag of every ray of an oracle trace o:
    warm_sensitivity at eta = 2^-45 above half the model's tau bar, tau floored at 1e-6"""
    r = rays(O, key, mode, pk)
    sens = oracle_plasma(O, r["pk"]).warm_sensitivity(r["xp"], r["Np"], omega(key), mode, DS, o["steps"],
                                                      iwarm=IWARM[model], eta=ETA)
    return ~(sens / np.maximum(np.abs(o["state"][:, 6]), TAU_FLOOR) <= 0.5 * BAR_TAU[model])


def stage_points(O, key, mode, every=25, pk=None):
    """(omega, X, Y, |N|, N_par, Te, 1 / |dD/dN|) rows at the oracle's end states of cold
    traces of 0, every, 2 every ... steps along a scenario's rays: the inputs the warm
    alpha sees along them.  Row i * n_rays + r is ray r after i * every steps."""
    r, om = rays(O, key, mode, pk), omega(key)
    op = oracle_plasma(O, r["pk"])
    rows = []
    for k in range(0, SCENARIOS[key]["n_steps"] + 1, every):
        st = op.trace(r["xp"], r["Np"], om, mode, DS, k, absorption=0)["state"] if k else np.hstack([r["xp"], r["Np"]])
        for i in range(len(st)):
            x, N = st[i, :3], st[i, 3:6]
            X, Y, Npar, _ = op.eval_plasma(x, N, om)
            rows.append((om, X, Y, np.linalg.norm(N), Npar, op.T_e(x), 1.0 / op.grad_norm(x, N, om, mode)))
    return np.array(rows)
