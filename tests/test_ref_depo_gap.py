"""The reference deposition (make_ray's splines, oracle/deposition_ref.py) of a
ray that starts inside an absorbing plasma, on the oracle's samples alone, CPU.

tests/test_gpu_skip_configs.py traces rays advanced 600 and 1200 cold steps
with their vacuum launch point kept: make_ray's vectors then run (0, dP/ds = 0),
(s0, 0), (s0 + ds, d1), (s0 + 2 ds, d2), ... with s0 = 0.36 - 0.42 m and ds = 1e-4 m.
The not-a-knot cubics of dP/ds and of psi over the gap [0, s0] are fixed by the
first samples past s0, each entering with a Lagrange factor of up to
0.375 (s0 / ds)^2 = 7e6 inside the gap.  Where d1 > 0 (25 keV, 120 GHz:
absorption is on at the start point, d1 = 2e-5 m^-1) the dP/ds cubic swings to
~100 m^-1 in the gap, the shells whose boundaries the psi cubic crosses there
collect power the ray never lost, and the last bits of the first psi samples
move those ~100 roots: the ray is outside the algorithm's domain, and its P_dep
is not reproducible to 1e-9 even by the reference itself.  Such rays are told
from the ray -- deposited above absorbed -- and this test holds that criterion
to the reference's own spline: it flags exactly the rays whose P_dep a 3e-14
nudge of the start point moves past the bar."""
import numpy as np
import pytest

DS = 1e-4


def ill_posed(P_dep, tau):
    """deposited above absorbed (1 - exp(-tau)) by more than 1e-6 of the unit power: well-posed
    rays deposit at most what they absorbed (what leaves the grid's shells is not deposited)"""
    return np.asarray(P_dep) - (1.0 - np.exp(-np.asarray(tau))) > 1e-6


def state_eps(a, b):
    """relative difference of two end states, x and N each against its vector's length"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    return np.maximum(np.abs(a[:, :3] - b[:, :3]).max(1) / np.linalg.norm(a[:, :3], axis=1),
                      np.abs(a[:, 3:6] - b[:, 3:6]).max(1) / np.linalg.norm(a[:, 3:6], axis=1))


@pytest.fixture(scope="module")
def rays(T, O):
    """four rays of the 25 keV 120 GHz X-mode fan, from vacuum and advanced 1200 steps: per ray the
    reference P_dep, tau and end state from the oracle's samples, at the start point as it is and
    nudged by 2^-45 and -2^-44 of itself"""
    import deposition_ref as D
    from torj_hip import synthetic as S

    s = S.SETUP
    eq = S.circular_tokamak(Te0=25e3)
    hp, op = T.Plasma(*S.plasma_args(eq)), O.OraclePlasma(*S.plasma_args(eq))
    f, mode = 120e9, 1
    om = 2 * np.pi * f
    N0 = T.pol_tor_angles_2_vector(s["steering_angle_pol"], s["steering_angle_tor"])
    pos, dirs, w = T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"],
                                            s["inverse_curvature_radius"], f, N_rings=6, min_azimuthal_points=5)
    idx = np.array([0, 85, 119, 170])
    xp, Np, s0, st = T.ray_entry(hp, pos[idx], dirs[idx], om, mode)
    assert (st == 0).all()
    grid = np.linspace(0, 1, 300)
    out = []
    for k in (0, 1200):
        start = np.hstack([xp, Np])
        if k:
            start = op.trace(xp, Np, om, mode, DS, k, absorption=False)["state"][:, :6]
        for n, i in enumerate(idx):
            row = dict(k=k, s0=s0[n] + k * DS, P=[], state=[])
            for nudge in (0.0, 2.0 ** -45, -2.0 ** -44):
                o = op.trace(start[n:n + 1, :3] * (1 + nudge), start[n:n + 1, 3:6], om, mode, DS, 3000,
                             chunk_steps=30, psi_grid=grid, P_min=5e-2, samples=True, s0=np.array([row["s0"]]))
                sv, psi, dpds = D.ray_vectors(pos[i], row["s0"], DS, o["steps"][0], o["samples"][0],
                                              op.evaluate("psi", pos[i]))
                row["P"].append(D.power_deposition_profile(sv, psi, dpds, grid, op.volume)[1])
                row["state"].append(o["state"][0].copy())
            row["d1"] = dpds[2]
            out.append(row)
    return out


def test_reference_deposition_across_a_launch_gap(rays):
    """From vacuum (dP/ds = 0 at the entry): deposited <= absorbed, and P_dep moves by less than the
    1e-9 bar under the nudges (measured 2e-14 - 7e-14, about the nudge itself).  Advanced 1200 steps
    (dP/ds > 0 at the start): the criterion flags the ray, the reference's own P_dep exceeds what
    the ray absorbed (1.2 - 1.6 against 0.7), and under the same nudges it misses 1e-9 (measured
    up to 8e-9: 1e5 per unit of trajectory difference against 1 from vacuum)."""
    worst = 0.0
    for r in rays:
        P, st = r["P"], r["state"]
        tau = st[0][6]
        ill = bool(ill_posed(P[0], tau))
        d = [abs(P[0] - P[j]) for j in (1, 2)]
        eps = [float(state_eps(st[0], st[j])[0]) for j in (1, 2)]
        print(f"advance {r['k']}: s0 {r['s0']:.3f} dP/ds at the first step {r['d1']:.2e}, P_dep {P[0]:.6f} absorbed "
              f"{1 - np.exp(-tau):.6f}, ill-posed {ill}; nudged: " +
              ", ".join(f"dP_dep {a:.1e} at eps {e:.1e} ({a / e:.1e} per unit)" for a, e in zip(d, eps)))
        assert ill == (r["k"] == 1200)
        assert all(0 < e < 1e-12 for e in eps)
        if ill:
            assert r["d1"] > 0
            worst = max(worst, *d)
        else:
            assert max(d) <= 1e-9, (r["k"], d)
    assert worst > 1e-9, worst
