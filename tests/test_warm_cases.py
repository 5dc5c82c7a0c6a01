"""The preconditions of tests/test_gpu_warm_paths.py, on the CPU oracle alone, so that the
GPU tests cannot pass vacuously: the scenarios of tests/warm_cases.py are what their
table says (statuses, tau ranges widened by 10 %, Y crossing 1, the Larmor orders that
decide which warm alpha kernel takes a point), the oracle's a-priori conditioning flag
(tests/test_gpu_c5.py) leaves every ray in, the oracle keeps B -> -B with a warm alpha
that takes N_par signed, and the host build of torj_warm.hpp (libwarm_host.so: the
source the trace kernels run) agrees with the oracle's C alpha at stage points along
the rays -- so that a GPU mismatch on these scenarios points at device-only code or at
the trace plumbing, not at the warm mathematics."""
import ctypes as C

import numpy as np
import pytest

import warm_cases as W
from test_warm_host import H, _d  # noqa: F401  (H: the host build of torj_warm.hpp)

C_LIGHT = 2.99792458e8
ALL = W.PAIRS + [("F", 1)]
ALL_IDS = W.PAIR_IDS + ["F-X"]


def _in_range(v, rng):
    return rng[0] * 0.9 <= v.min() and v.max() <= rng[1] * 1.1


@pytest.mark.parametrize("model", [2, 3])
@pytest.mark.parametrize("key,mode", ALL, ids=ALL_IDS)
def test_scenario_is_what_the_table_says(O, key, mode, model):
    """Every ray enters with status 0 (warm_cases.rays asserts it); the end statuses, the
    optical depths and the conditioning flag of the oracle's trace."""
    sc = W.SCENARIOS[key]
    o = W.oracle_trace(O, key, mode, model)
    tau = o["state"][:, 6]
    print(f"{key} {sc['name']} mode {mode:+d} model {model}: statuses "
          f"{dict(zip(*np.unique(o['status'], return_counts=True)))}, steps {o['steps'].min()} - {o['steps'].max()}, "
          f"tau {tau.min():.4g} - {tau.max():.4g}")
    if key == "B":
        assert (o["status"] == W.ABSORBED).all()
        assert 0.9 * 830 <= o["steps"].min() and o["steps"].max() <= 1.1 * 830 and o["steps"].max() < sc["n_steps"]
        o2 = W.oracle_trace(O, key, mode, model, P_min=1e-12)
        assert (o2["status"] == W.OK).all() and (o2["steps"] == sc["n_steps"]).all()
        assert _in_range(o2["state"][:, 6], sc["tau_no_stop"][mode]), o2["state"][:, 6]
    elif key == "F":
        n = W.rays(O, key, mode)["n_fan"]
        assert 65 <= len(tau) <= 127 and len(tau) % 64 != 0
        assert (o["status"][:n] == W.ABSORBED).all() and (o["status"][n:] == W.LEFT_PLASMA).all()
        lo, hi = W.F_STOPS[model]
        assert 0.9 * lo <= o["steps"][:n].min() and o["steps"][:n].max() <= 1.1 * hi
        # rays of one wave stop at differing blocks, and before the outward rays' own stops
        assert len(np.unique(o["steps"][:n])) >= 4 and o["steps"][n:].max() < o["steps"][:n].min()
    else:
        assert (o["status"] == W.OK).all() and (o["steps"] == sc["n_steps"]).all()
    if sc["tau"]:
        assert _in_range(tau, sc["tau"][mode]), (tau.min(), tau.max())
    fl = W.flagged(O, key, mode, model, o)
    print(f"{key} mode {mode:+d} model {model}: {fl.sum()} of {len(fl)} rays flagged")
    assert fl.mean() <= 0.05, fl.mean()


def test_b_crosses_the_fundamental(O):
    """Y passes 1 along ray 0 of B: R5's sox flip and warmdisp's yg > 1 branch are reached"""
    n = len(W.rays(O, "B", -1)["w"])
    Y = W.stage_points(O, "B", -1)[::n, 2]
    print(f"B ray 0: Y {Y.min():.4f} - {Y.max():.4f}")
    assert Y.min() < 1.0 < Y.max()
    assert Y[0] < 1.0 < Y[-1]


@pytest.mark.parametrize("model", [2, 3])
def test_b_engages_the_adaptive_power_clamp(O, model):
    """warm_cases.CLAMP on B in the oracle: some saved P = exp(-tau) are exactly 0 (the clamp of
    the reference's ContinuousCallback projected an overshoot back), none is negative or NaN,
    and the rays it caught stop ABSORBED at the next chunk boundary."""
    o = W.oracle_trace(O, "B", -1, model, n_steps=W.CLAMP_CAP, **W.CLAMP)
    saved = np.arange(W.CLAMP_CAP)[None, :] < o["steps"][:, None]
    P = np.exp(-o["traj"][:, :, 3])
    print(f"B model {model}, dtmax 2 cm: statuses {dict(zip(*np.unique(o['status'], return_counts=True)))}, steps "
          f"{o['steps'].min()} - {o['steps'].max()}, saved P = 0: {(P[saved] == 0).sum()}")
    assert (P[saved] >= 0.0).all() and (P[saved] == 0.0).any()
    assert W.ABSORBED in o["status"].tolist() and o["steps"].max() < W.CLAMP_CAP


@pytest.mark.parametrize("key,mode", [("D", 1), ("D", -1), ("E", 1)], ids=["D-X", "D-O", "E-X"])
def test_larmor_orders(O, key, mode):
    """warm_ref.larmornumber along ray 0: D at 4 or above at every sampled point (the alpha
    takes lrm = min(5, .): every point is deferred to k_alpha_warm_big), E at 3 and 4, about
    half each (k_alpha_warm_pts defers part of a wave)."""
    import warm_ref

    n = len(W.rays(O, key, mode)["w"])
    p = W.stage_points(O, key, mode)[::n]
    mu = warm_ref.ME * warm_ref.C * warm_ref.C / (p[:, 5] * warm_ref.E)
    lr = np.array([warm_ref.larmornumber(y, npl, m) for y, npl, m in zip(p[:, 2], p[:, 4], mu)])
    print(f"{key} mode {mode:+d} ray 0: larmornumber {dict(zip(*np.unique(lr, return_counts=True)))}")
    if key == "D":
        assert (lr >= 4).all()
    else:
        assert set(lr.tolist()) == {3, 4}
        assert 0.25 <= (lr == 3).mean() <= 0.75


@pytest.mark.parametrize("iwarm,bar", [(3, 1e-8), (1, 1e-7)])
@pytest.mark.parametrize("key,mode", ALL, ids=ALL_IDS)
def test_host_alpha_matches_oracle_along_the_rays(H, O, key, mode, iwarm, bar):  # noqa: F811
    """wh_alpha_warm at the oracle's cold end states every 25 steps along the scenario's rays
    (F: every 50) against O.alpha_warm, by test_warm_host.py test_alpha_warm_matches_oracle's
    error measure: |d alpha| over |alpha| + 1e-9 of 2 |N_perp^2| (omega / c) / |dD/dN|, the
    rounding floor of Im(N_perp^2); the finite / non-finite pattern exact."""
    p = W.stage_points(O, key, mode, every=50 if key == "F" else 25)
    n = len(p)
    cols = [np.ascontiguousarray(p[:, k]) for k in range(7)]
    a, n2 = np.zeros(n), np.zeros(2 * n)
    H.wh_alpha_warm(n, *[_d(c) for c in cols], mode, iwarm, a.ctypes.data_as(C.POINTER(C.c_double)),
                    n2.ctypes.data_as(C.POINTER(C.c_double)))
    ar, nr = np.zeros(n), np.zeros(n, complex)
    for i in range(n):
        ar[i], nr[i] = O.alpha_warm(*p[i], mode, iwarm)
    assert np.array_equal(np.isfinite(a), np.isfinite(ar))
    fin = np.isfinite(ar)
    floor = 1e-9 * 2 * np.abs(nr) * p[:, 0] / C_LIGHT * p[:, 6]
    e = (np.abs(a - ar) / (np.abs(ar) + floor + 1e-300))[fin]
    print(f"{key} mode {mode:+d} iwarm {iwarm}: {n} points ({(~fin).sum()} non-finite in both), host vs oracle alpha "
          f"max {e.max():.2e}, |alpha| up to {np.abs(ar[fin]).max():.3g} /m")
    assert fin.sum() > 0.9 * n and np.abs(ar[fin]).max() > 0
    assert e.max() <= bar, e.max()


@pytest.mark.parametrize("model", [2, 3])
@pytest.mark.parametrize("mode", [1, -1])
def test_oracle_keeps_field_reversal_with_a_warm_alpha(O, mode, model):
    """C through the reversed field (sigma = -1) gives sigma = +1's end states in the oracle
    alone, at the GPU test's bars: statuses and steps exact, x, N 1e-10, tau at the model's
    bar.  N_par changes sign with B, and the warm alpha takes it signed."""
    import shaped_eq as E

    ra, rb = W.rays(O, "C", mode), W.rays(O, "C", mode, "s-")
    assert np.abs(ra["xp"] - rb["xp"]).max() < 1e-12 and np.abs(ra["Np"] - rb["Np"]).max() < 1e-12
    pa, pb = W.oracle_plasma(O, "s+"), W.oracle_plasma(O, "s-")
    na = pa.eval_plasma(ra["xp"][0], ra["Np"][0], W.omega("C"))[2]
    nb = pb.eval_plasma(rb["xp"][0], rb["Np"][0], W.omega("C"))[2]
    assert abs(na + nb) < 1e-12 and abs(na) > 0.2
    a, b = W.oracle_trace(O, "C", mode, model), W.oracle_trace(O, "C", mode, model, "s-")
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["steps"], b["steps"])
    ex, eN, et = E.trace_errs(b["state"], a["state"], W.TAU_FLOOR)
    print(f"oracle C mode {mode:+d} model {model}, B -> -B: x {ex:.2e} N {eN:.2e} tau {et:.2e}, bit-identical "
          f"{np.array_equal(a['state'], b['state'])}")
    assert ex <= 1e-10 and eN <= 1e-10 and et <= W.BAR_TAU[model], (ex, eN, et)
    assert _in_range(b["state"][:, 6], W.SCENARIOS["C"]["tau"][mode])
