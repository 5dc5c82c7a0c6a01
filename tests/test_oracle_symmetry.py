"""Exact symmetries of the physics on the CPU oracle alone (oracle/torj_oracle.c),
on the shaped equilibrium of tests/shaped_eq.py: GPU parity is measured against
this oracle, so an error the two share is invisible there; a symmetry needs no
second implementation.  Only rounding separates the two sides of each, so the
project's 1e-10 parity bar (statuses and steps exact) is the criterion, and the
measured discrepancy is printed (tests/test_gpu_geometry.py prints the GPU's
beside it).

  rotation  a launch rotated about the Z axis by 2.3 rad (|y| ~ |x| or larger), positions and
            directions alike, gives the rotated trace;
  reversal  the plasma with B -> -B gives the same trace (the dispersion and the
            Albajar absorption depend on |B| and N_par^2);
  mirror    on circular_tokamak() (psi and box symmetric in Z) the launch mirrored
            in Z = 0 gives the mirrored trace -- through the plasma's mirror image,
            which has the toroidal field reversed (B is a pseudovector: the image of
            (B_R, B_phi, B_Z)(R, Z) is (-B_R, -B_phi, B_Z)(R, -Z), and circular_tokamak()
            has B_R odd and B_Z, B_phi even in Z).  Through the same plasma the
            mirrored fan's N_par differs wherever a ray has a toroidal component, and
            the traces differ by 3e-3;
  points    B_spline and grad_lambda rotate covariantly at random toroidal angles.

46-ray fans (n_rings 3), 92.5 GHz, both modes, 6 000 steps of 1e-4 m, termination
checks every 60, 200 shells.  And the ray entry's finding: a rounding-dependent
ENTRY_FAIL of first_point, which depended on the toroidal angle."""
import numpy as np
import pytest

import shaped_eq as E

DS, N_STEPS, CHUNK = 1e-4, 6000, 60
GRID = np.linspace(0.0, 1.0, 200)
TOL = 1e-10
# the toroidal angles of the entry scan: 0, the rotation of the trace tests, 40 random
ENTRY_PHIS = np.concatenate([[0.0, E.PHI_ROT], np.random.default_rng(0).uniform(-np.pi, np.pi, 40)])


@pytest.fixture(scope="module")
def ctx(O):
    from torj_hip import synthetic as S

    plasmas = {1: O.OraclePlasma(*E.shaped_args(sigma=1.0)), -1: O.OraclePlasma(*E.shaped_args(sigma=-1.0)),
               "circ": O.OraclePlasma(*S.plasma_args(S.circular_tokamak())),
               "circ_image": O.OraclePlasma(*S.plasma_args(E.mirror_image(S.circular_tokamak())))}
    return dict(O=O, plasmas=plasmas, runs={})


def oracle_entry(op, pos, dirs, mode, omega=E.OMEGA):
    """or_ray_entry ray by ray: (status, x_plasma, N_plasma, s0) arrays"""
    r = [op.ray_entry(pos[i], dirs[i], omega, mode) for i in range(len(pos))]
    return (np.array([q[0] for q in r]), np.array([q[1] for q in r]), np.array([q[2] for q in r]),
            np.array([q[3] for q in r]))


def oracle_run(ctx, plasma, launch, mode, phi=0.0, mirrored=False, n_rings=3):
    """entry + trace of one fan on one of the context's plasmas, kept for the tests that share it"""
    key = (plasma, launch, mode, phi, mirrored, n_rings)
    if key not in ctx["runs"]:
        O, op = ctx["O"], ctx["plasmas"][plasma]
        pos, dirs, w = E.fan(O, launch, n_rings, 5, phi)
        if mirrored:
            pos, dirs = E.mirror(pos), E.mirror(dirs)
        st, xp, Np, s0 = oracle_entry(op, pos, dirs, mode)
        assert (st == 0).all(), (key, st)
        o = op.trace(xp, Np, E.OMEGA, mode, DS, N_STEPS, chunk_steps=CHUNK, psi_grid=GRID, weights=w)
        o.update(xp=xp, Np=Np, s0=s0, pos=pos, dirs=dirs, w=w)
        ctx["runs"][key] = o
    return ctx["runs"][key]


def compare(a, b, state_b, what):
    """b's trace, its end states brought into a's frame (state_b), against a's at
    _compare_trace's bars; the shell profile and the rays' deposited power to 1e-10
    of their maxima.  Prints and returns the discrepancies."""
    assert np.array_equal(a["status"], b["status"]), what
    assert np.array_equal(a["steps"], b["steps"]), what
    ex, eN, et = E.trace_errs(state_b, a["state"])
    ed = np.abs(a["dP"] - b["dP"]).max() / max(np.abs(a["dP"]).max(), 1e-300)
    ep = np.abs(a["Pdep"] - b["Pdep"]).max() / max(np.abs(a["Pdep"]).max(), 1e-300)
    print(f"oracle {what}: x {ex:.2e} N {eN:.2e} tau {et:.2e} dP {ed:.2e} P_dep {ep:.2e}; statuses "
          f"{dict(zip(*np.unique(a['status'], return_counts=True)))}, tau {a['state'][:, 6].min():.3g} - "
          f"{a['state'][:, 6].max():.3g}")
    assert max(ex, eN, et) < TOL, (what, ex, eN, et)
    assert ed <= TOL and ep <= TOL, (what, ed, ep)
    return ex, eN, et, ed


@pytest.mark.parametrize("mode", [1, -1])
@pytest.mark.parametrize("name", sorted(E.LAUNCHES))
def test_rotation(ctx, name, mode):
    a = oracle_run(ctx, 1, E.LAUNCHES[name], mode)
    b = oracle_run(ctx, 1, E.LAUNCHES[name], mode, phi=E.PHI_ROT)
    # the rotated fan is what it says: |y| comparable to |x|, or larger, at its entry points
    assert (np.abs(b["xp"][:, 1]) > 0.9 * np.abs(b["xp"][:, 0])).all()
    assert np.abs(E.rotz(a["xp"], E.PHI_ROT) - b["xp"]).max() < 1e-12
    compare(a, b, E.rot_state(b["state"], -E.PHI_ROT), f"rotation {name} mode {mode:+d}")


@pytest.mark.parametrize("mode", [1, -1])
@pytest.mark.parametrize("name", sorted(E.LAUNCHES))
def test_field_reversal(ctx, name, mode):
    a = oracle_run(ctx, 1, E.LAUNCHES[name], mode)
    b = oracle_run(ctx, -1, E.LAUNCHES[name], mode)
    assert np.abs(a["xp"] - b["xp"]).max() < 1e-12 and np.abs(a["Np"] - b["Np"]).max() < 1e-12
    compare(a, b, b["state"], f"reversal {name} mode {mode:+d}")


@pytest.mark.parametrize("mode", [1, -1])
def test_mirror_on_circular(ctx, mode):
    from torj_hip import synthetic as S

    s = S.SETUP
    setup = ((s["R0"], 0.0, s["z0"]), np.rad2deg(s["steering_angle_pol"]), np.rad2deg(s["steering_angle_tor"]))
    a = oracle_run(ctx, "circ", setup, mode)
    b = oracle_run(ctx, "circ_image", setup, mode, mirrored=True)
    assert (b["xp"][:, 2] < 0).all() and (a["xp"][:, 2] > 0).all()  # the mirrored fan comes from below
    compare(a, b, E.mirror_state(b["state"]), f"mirror SETUP mode {mode:+d}")


def test_workload_lfs_down_crosses_the_layer_and_the_others_do_not(ctx):
    """the workload, on the oracle's own results: X-mode from the low-field side
    crosses the second-harmonic layer (tau > 5 on every ray), the top and the
    high-field-side launches end OK after all 6 000 steps"""
    a = oracle_run(ctx, 1, E.LAUNCHES["lfs_down"], 1)
    assert a["state"][:, 6].min() > 5.0
    for name in ("top", "hfs"):
        for mode in (1, -1):
            o = oracle_run(ctx, 1, E.LAUNCHES[name], mode)
            assert (o["status"] == 0).all() and (o["steps"] == N_STEPS).all()
    # the launches differ where the circular fan does not: lower half plane, sizeable N_par
    assert (a["xp"][:, 2] < 0).all()
    X, Y, Npar, b = ctx["plasmas"][1].eval_plasma(a["xp"][0], a["Np"][0], E.OMEGA)
    assert abs(Npar) > 0.15


def test_fields_and_ray_equations_rotate_covariantly(ctx):
    """B_spline(R x) = R B_spline(x) and grad_lambda(R x, R N) = R grad_lambda(x, N) for
    rotations R about Z by random angles, at random points of the shaped plasma's box, both
    field directions and both modes.

    B and dx/ds, the first half of du: 1e-13 of the vector, at every point of the box.

    dN/ds, the second half, does NOT meet 1e-13 of the vector, and is held to a scaled bar
    instead (a deviation from the plain figure, measured below).  It is -grad Lambda /
    |dLambda/dN|, and grad Lambda carries X grad ln n_e: a sum of 16 spline terms of size
    |ln n_e| / h each (ln n_e ~ 45, h = 0.04: ~1 100) that cancel to a gradient of order 1,
    so its rounding is relative to those terms, not to the result.  The bar is 1e-13 of
    max(|dN/ds|, X |ln n_e| / h) at the points inside the plasma (psi <= 1, where rays are
    integrated; outside, ln n_e falls steeply to -900 and the stencil's coefficients exceed
    the local value, so no local scale is sound there and the half is only printed).
    Measured on the oracle: up to 1.25e-12 of |dN/ds| inside the plasma, 6.6e-15 of the
    scaled bar's scale; a sign or convention error shows at 1e-3 or more."""
    rng = np.random.default_rng(11)
    n = 400
    R, Z = rng.uniform(1.0, 2.6, n), rng.uniform(-1.2, 1.1, n)
    x = np.stack([R, np.zeros(n), Z], 1)
    N = rng.normal(size=(n, 3))
    N *= (rng.uniform(0.3, 0.95, n) / np.linalg.norm(N, axis=1))[:, None]
    phi = rng.uniform(-np.pi, np.pi, n)
    worst = dict(B=0.0, dx=0.0, dN_scaled=0.0, dN_raw_in=0.0, dN_raw_out=0.0)
    finite = inside = 0
    hR, hZ = (np.diff(E.shaped_tokamak()[k])[0] for k in ("R_coords", "Z_coords"))
    inv_h = max(1.0 / hR, 1.0 / hZ)
    for sigma in (1, -1):
        op = ctx["plasmas"][sigma]
        for i in range(n):
            xr, Nr = E.rotz(x[i], phi[i]), E.rotz(N[i], phi[i])
            B, Br = op.B_spline(x[i]), op.B_spline(xr)
            eB = np.abs(E.rotz(B, phi[i]) - Br).max() / np.linalg.norm(B)
            worst["B"] = max(worst["B"], eB)
            assert eB <= 1e-13, (sigma, i, eB)
            in_plasma = op.evaluate("psi", x[i]) <= 1.0
            for mode in (1, -1):
                du = op.grad_lambda(x[i], N[i], E.OMEGA, mode)
                dur = op.grad_lambda(xr, Nr, E.OMEGA, mode)
                if not np.all(np.isfinite(du)):
                    assert np.array_equal(np.isfinite(du), np.isfinite(dur))
                    continue
                finite += 1
                ex = np.abs(E.rotz(du[:3], phi[i]) - dur[:3]).max() / np.linalg.norm(du[:3])
                worst["dx"] = max(worst["dx"], ex)
                assert ex <= 1e-13, (sigma, i, mode, ex)
                dN = np.abs(E.rotz(du[3:], phi[i]) - dur[3:]).max()
                raw = dN / max(np.linalg.norm(du[3:]), 1e-300)
                if not in_plasma:
                    if np.linalg.norm(du[3:]) > 0:
                        worst["dN_raw_out"] = max(worst["dN_raw_out"], raw)
                    continue
                inside += 1
                worst["dN_raw_in"] = max(worst["dN_raw_in"], raw)
                terms = op.eval_plasma(x[i], N[i], E.OMEGA)[0] * abs(np.log(op.n_e(x[i]))) * inv_h
                e = dN / max(np.linalg.norm(du[3:]), terms, 1e-300)
                worst["dN_scaled"] = max(worst["dN_scaled"], e)
                assert e <= 1e-13, (sigma, i, mode, e)
    assert inside > n // 2 and finite > 2 * n  # a third of the box is plasma; two fields, two modes
    print(f"oracle covariance at {n} points x 2 fields ({finite} finite du, {inside} inside the plasma): "
          f"B {worst['B']:.2e}, dx/ds {worst['dx']:.2e} of the vector (bar 1e-13, every point); dN/ds "
          f"{worst['dN_scaled']:.2e} of max(|dN/ds|, X |ln n_e| / h) (bar 1e-13, inside), "
          f"{worst['dN_raw_in']:.2e} of |dN/ds| inside and {worst['dN_raw_out']:.2e} outside (not held)")


def test_entry_does_not_depend_on_the_toroidal_angle(ctx, T):
    """first_point bisects to machine precision, so psi at its result can exceed
    psi_prof_max by one rounding error; the reference's step 2 (psi - psi_max) N0 is then
    below an ulp of the coordinates and make_ray's psi <= psi_max check refused the ray:
    ENTRY_FAIL on 12 of the 19 572 (ray, angle, mode) triples of the top launch's fans
    (46 and 187 rays) over these 42 angles in the oracle.  The product's entry is the same
    algorithm with another rounding of psi; no ray was found that it refused,
    so there the fix is a guard this test does not reach.  Both now take the bracket's
    inside end in that case.  Every ray of every launch enters, at every angle, in the oracle and in the
    product's host entry alike, and both give the rotated entry state."""
    hp = T.Plasma(*E.shaped_args())
    op = ctx["plasmas"][1]
    launches = dict(E.LAUNCHES, edge=E.EDGE_LAUNCH)
    for name, launch in sorted(launches.items()):
        ref = None
        for phi in ENTRY_PHIS:
            pos, dirs, _w = E.fan(ctx["O"], launch, 3, 5, phi)
            for mode in (1, -1):
                st, xp, Np, s0 = oracle_entry(op, pos, dirs, mode)
                h = T.ray_entry(hp, pos, dirs, E.OMEGA, mode)
                assert (st == 0).all() and (h[3] == 0).all(), (name, phi, mode, st, h[3])
                assert np.abs(h[0] - xp).max() < 1e-12 and np.abs(h[1] - Np).max() < 1e-12
                assert np.abs(h[2] - s0).max() < 1e-12
                assert (np.array([op.evaluate("psi", p) for p in xp]) <= op.psi_prof_max).all()
                back = (E.rotz(xp, -phi), E.rotz(Np, -phi), s0)
                if phi == 0.0:
                    ref = ref or {}
                    ref[mode] = back
                else:
                    for a, b in zip(ref[mode], back):
                        assert np.abs(a - b).max() < 1e-12, (name, phi, mode)
