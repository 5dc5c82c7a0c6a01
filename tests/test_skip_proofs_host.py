"""The Albajar skip proofs on CPU, pointwise over their input domain, in both
forms of the node exponent (TORJ_NODE_GAMMA_LIN 1, the default, and 0):

* the block zero box (torj_math.hpp ZBox, zero_box_add, zero_box_flag; the
  proof is stated at torj_k_traj.hpp): a set flag means abs_albajar_fast_body
  returns a zero at every point the box covers, with the skips on and off;
* the tiny-alpha skip (tiny_harmonic): alpha moves by at most tiny_alpha per
  skipped harmonic at single points, not only along the headline fan's traces.

Host build of tests/native/skip_proofs_host.hip (the device takes v_max_f64 /
v_min_f64 where the host takes fmax / fmin; NaN inputs are the box's chk word's
business in both)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_h3_fast_host import _edges, _random, _ulps

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
K_MU_TE = 9.1093837015e-31 * 2.99792458e8 ** 2 / 1.602176634e-19  # mu Te (albajar_pre), eV
LN20 = 2.9957322735539909
N_BOXES = 200000
# 200 000 boxes per mode: single points, 8-point boxes and whole 60-step blocks
# (240 stage points)
K_SHARE = ((1, 80000), (8, 110000), (240, 10000))
# (negl_skip, tiny_alpha): the default, the exact leg, the reference's full work
VARIANTS = ((1, 1e-20), (1, 0.0), (0, 0.0))


def _p(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module", params=[1, 0], ids=["gamma_lin1", "gamma_lin0"])
def H(request):
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", f"libskip_proofs_host{request.param}.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # libwarm_host.so's flags (tests/native/Makefile), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           f"-DTORJ_NODE_GAMMA_LIN={request.param}",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "skip_proofs_host.hip")])
    L = C.CDLL(out)
    L.sp_setup.argtypes = [C.c_int, _dp, _dp]
    L.sp_flags.argtypes = [C.c_int, C.c_int] + [_dp] * 4 + [_ip]
    L.sp_alpha.argtypes = [C.c_int] + [_dp] * 5 + [C.c_double, C.c_int, C.c_int, C.c_double, _dp]
    L.sp_alpha_pts.argtypes = [C.c_int] + [_dp] * 5 + [C.c_double, C.c_int, C.c_double, _dp]
    assert L.sp_gamma_lin() == request.param
    t, w = np.polynomial.legendre.leggauss(24)
    L.sp_setup(24, _p(np.ascontiguousarray(t)), _p(np.ascontiguousarray(w)))
    return L


def _flags(H, P):
    """P: dict of (nb, k) arrays lnTe, Y, Npar, N2 -> zero_box_flag per box"""
    nb, k = P["lnTe"].shape
    cols = [np.ascontiguousarray(P[f], dtype=float) for f in ("lnTe", "Y", "Npar", "N2")]
    flag = np.zeros(nb, dtype=np.int32)
    H.sp_flags(nb, k, *[_p(c) for c in cols], flag.ctypes.data_as(_ip))
    return flag == 1


def _alpha(H, P, sel, om, mode, negl, tiny):
    """alpha at every point of the boxes sel of P, flat"""
    cols = [np.ascontiguousarray(P[f][sel].ravel(), dtype=float) for f in ("lnTe", "Y", "Npar", "N2", "X")]
    out = np.full(len(cols[0]), np.nan)
    H.sp_alpha(len(out), *[_p(c) for c in cols], om, mode, negl, tiny, _p(out))
    return out


def _boxes(nb, k, rng):
    """nb boxes of k points around random centres, and k fresh points per box
    drawn from the ranges the added points span (what the box records: ln Te up
    to its maximum, Y between its extremes, |N_par| up to its maximum, N_perp^2
    down to its minimum) but not added.  Relative widths log-uniform 1e-12 - 0.3,
    drawn per box and input."""
    c = dict(Te=np.exp(rng.uniform(0.0, np.log(3e4), nb)), Y=rng.uniform(0.05, 1.5, nb),
             Npar=rng.uniform(-0.99, 0.99, nb), Np2=np.exp(rng.uniform(np.log(1e-6), np.log(1.2), nb)))
    wd = {f: np.exp(rng.uniform(np.log(1e-12), np.log(0.3), nb)) for f in c}
    v = {f: c[f][:, None] * (1.0 + wd[f][:, None] * rng.uniform(-1.0, 1.0, (nb, k))) for f in c}
    P = dict(lnTe=np.log(v["Te"]), Y=v["Y"], Npar=v["Npar"], N2=v["Npar"] ** 2 + v["Np2"],
             X=rng.uniform(0.0, 1.2, (nb, k)))
    lo = {f: v[f].min(1)[:, None] for f in v}
    hi = {f: v[f].max(1)[:, None] for f in v}
    u = {f: lo[f] + (hi[f] - lo[f]) * rng.uniform(0.0, 1.0, (nb, k)) for f in v}
    F = dict(lnTe=np.minimum(np.log(u["Te"]), P["lnTe"].max(1)[:, None]), Y=u["Y"], Npar=u["Npar"],
             N2=u["Npar"] ** 2 + u["Np2"], X=rng.uniform(0.0, 1.2, (nb, k)))
    return P, F


def _assert_zero(H, P, sel, om, mode, what):
    """alpha is a zero of either sign, never NaN, at every point of the boxes
    sel, in all three variants"""
    if not np.any(sel):
        return
    for negl, tiny in VARIANTS:
        with np.errstate(all="ignore"):
            a = _alpha(H, P, sel, om, mode, negl, tiny)
        bad = ~(a == 0.0)
        if bad.any():
            i = np.flatnonzero(bad)[:3]
            rows = {f: P[f][sel].ravel()[i] for f in ("lnTe", "Y", "Npar", "N2", "X")}
            raise AssertionError(f"{what}: flag set, alpha {a[i]} (negl_skip {negl}, tiny {tiny:g}) at {rows}")


@pytest.mark.parametrize("mode", [1, -1])
def test_zero_box_sound_on_random_boxes(H, mode):
    """Soundness: zero_box_flag => alpha == 0 (either sign), not NaN, at every
    added point and at as many fresh points of the box's ranges, for negl_skip 1
    with tiny_alpha 1e-20 and 0 and for negl_skip 0; and the flag is no empty
    promise: at least 10 000 of the 200 000 boxes are flagged with Te >= 20 eV
    somewhere in them (measured: about 47 000 in either mode)."""
    assert sum(n for _, n in K_SHARE) == N_BOXES
    rng = np.random.default_rng(20260 + mode)
    om = 2 * np.pi * 92.5e9
    n_flag = n_warm = 0
    for k, nb in K_SHARE:
        P, F = _boxes(nb, k, rng)
        fl = _flags(H, P)
        warm = fl & (P["lnTe"].max(1) >= LN20)
        print(f"mode {mode:+d} k {k}: {nb} boxes, flagged {fl.mean():.3f}, flagged and warm {warm.mean():.3f}")
        _assert_zero(H, P, fl, om, mode, f"k {k} added points")
        _assert_zero(H, F, fl, om, mode, f"k {k} fresh points")
        n_flag += int(fl.sum())
        n_warm += int(warm.sum())
    print(f"mode {mode:+d}: flagged share {n_flag / N_BOXES:.4f}, warm among flagged {n_warm / max(n_flag, 1):.4f}")
    assert n_warm >= 10000, n_warm


def _eps():
    """relative offsets from a threshold: within +-4 ulp, out to +-2e-9 across the
    proofs' 1e-9 margins, and +-3e-9, +-1e-8 beyond the two margins some
    inequalities carry (one on each side), so that every flag is seen to flip"""
    u = [k * 2.0 ** -52 for k in range(-4, 5)]
    r = [s * e for s in (-1, 1) for e in (5e-10, 1e-9 * (1 - 1e-6), 1e-9, 1e-9 * (1 + 1e-6), 2e-9,
                                          2e-9 * (1 + 1e-6), 3e-9, 1e-8)]
    return np.array(sorted(u + r))


def _threshold_points():
    """name -> rows (lnTe, Y, Npar, N2) placed across one inequality of
    zero_box_flag each, everything else held where the flag's other terms pass"""
    e = _eps()
    out = {}
    # Te = 20 eV with harmonic 2 on resonance: alpha > 0 from 20 eV on
    npar = 0.3
    sq = np.sqrt(1 - npar * npar)
    for tag, shift in (("", 0.0), (" at the flag's margin", -1e-9)):
        # (N_par = 0: gamma = 2 Y = 1.0001 on the whole ellipse, mu (gamma - 1) = 2.6)
        out["Te = 20 eV" + tag] = [(np.log(20.0 * (1 + x)) + shift, 0.5 * (1 + 1e-4), 0.0, 0.5) for x in e]
        out["Te = 20 eV" + tag] += [(v + shift, 0.5 * (1 + 1e-4), 0.0, 0.5) for v in _ulps(LN20, range(-4, 5))]
    # m Y = sqrt(1 - N_par^2): harmonic m absent below; at 40 eV the other
    # harmonic is absent (m = 3) or an exact zero (m = 2: 3 Y > (1 + delta)(1 + |N_par|))
    for m in (2, 3):
        out[f"{m} Y = sqrt(1 - N_par^2)"] = [(np.log(40.0), sq / m * (1 + x), npar, npar ** 2 + 0.5) for x in e]
    # m Y = (1 + 760 / mu)(1 + |N_par|): harmonic m an exact zero above; at 100 eV,
    # N_par 0.1, harmonic 2 is absent at the m = 3 threshold
    te, npar = 100.0, 0.1
    for m in (2, 3):
        y = (1 + 760.0 * te / K_MU_TE) * (1 + npar) / m
        out[f"{m} Y = (1 + 760 / mu)(1 + |N_par|)"] = [(np.log(te), y * (1 + x), s * npar, npar ** 2 + 0.5)
                                                         for x in e for s in (1, -1)]
    # N_par^2 = 1 and the flag's own bounds below it (1 - 1e-9; 1 - 1e-6 for the
    # square-root form of the node exponent), both signs, far above both zero thresholds
    out["N_par^2 = 1"] = [(np.log(40.0), 1.4, s * np.sqrt(t * (1 + x)), t * (1 + x) + 0.5)
                          for x in e for s in (1, -1) for t in (1.0, 1.0 - 1e-9, 1.0 - 1e-6)]
    # N_perp^2 = 0 and the flag's 1e-9 |N|^2
    npar = 0.3
    out["N_perp^2 = 0"] = [(np.log(40.0), 1.4, npar, npar ** 2 * (1 + x)) for x in e]
    out["N_perp^2 = 0"] += [(np.log(40.0), 1.4, npar, npar ** 2 / (1 - 1e-9) * (1 + x)) for x in e]
    out["N_perp^2 = 0"] += [(np.log(40.0), 1.4, npar, v) for v in _ulps(npar ** 2, range(-4, 5))]
    # ln Te = 700 (exp(ln Te) still finite) and the flag's own bound, 300, both harmonics absent
    out["ln Te = 700"] = [(700.0 * (1 + x), 0.1, 0.3, 0.59) for x in e]
    out["ln Te = 300"] = [(300.0 * (1 + x), 0.1, 0.3, 0.59) for x in e]
    return {k: np.array(v, dtype=float) for k, v in out.items()}


@pytest.mark.parametrize("mode", [1, -1])
def test_zero_box_sound_at_its_thresholds(H, mode):
    """Boxes within +-4 ulp and +-2e-9 relative of each inequality of the flag
    (Te = 20 eV, m Y = sqrt(1 - N_par^2) and m Y = (1 + 760 / mu)(1 + |N_par|)
    for m = 2, 3, N_par^2 = 1, N_perp^2 = 0, ln Te = 700 and the flag's own
    ln Te = 300): soundness on both sides, as single points and as boxes of a
    threshold point beside seven points well inside the flagged region; every
    threshold is crossed (the flag is set on one side of it and clear on the
    other) but ln Te = 700, where the flag refuses on both sides: up to there
    the flag once promised a zero where the body without its skips (negl_skip 0)
    overflows to NaN in albajar_finish, from ln Te = 368 on."""
    om = 2 * np.pi * 92.5e9
    rng = np.random.default_rng(5)
    for name, rows in _threshold_points().items():
        n = len(rows)
        for k in (1, 8):
            P = {f: np.repeat(rows[:, j][:, None], k, 1) for j, f in enumerate(("lnTe", "Y", "Npar", "N2"))}
            P["X"] = rng.uniform(0.0, 0.999, (n, k))
            if k == 8:
                # seven companions that keep every term of the flag passed: colder, a larger Y
                # above the zero thresholds, a smaller |N_par|, a larger N_perp^2
                up = not ("sqrt" in name or "Te" in name)
                P["lnTe"][:, 1:] -= rng.uniform(0.0, 0.5, (n, 7))
                # (below an absence threshold by 1 % at most: at m = 2 harmonic 3 must stay a zero)
                P["Y"][:, 1:] *= 1 + (0.05 if up else -0.01) * rng.uniform(0.0, 1.0, (n, 7))
                P["Npar"][:, 1:] *= rng.uniform(0.5, 1.0, (n, 7))
                P["N2"][:, 1:] = P["Npar"][:, 1:] ** 2 + (rows[:, 3] - rows[:, 2] ** 2)[:, None] + 0.1
                pos = rng.integers(0, 8, n)  # the threshold point at a random position
                for f in P:
                    a = P[f][np.arange(n), pos].copy()
                    P[f][np.arange(n), pos] = P[f][:, 0]
                    P[f][:, 0] = a
            fl = _flags(H, P)
            print(f"mode {mode:+d} k {k} {name}: {n} boxes, {int(fl.sum())} flagged")
            if name == "ln Te = 700":  # inside the refused range since the bound is 300
                assert not fl.any(), (name, k, fl)
            else:
                assert 0 < fl.sum() < n, (name, k, fl)
            _assert_zero(H, P, fl, om, mode, name)
    # the Te = 20 eV boxes are a live test: just above 20 eV alpha is not 0
    rows = _threshold_points()["Te = 20 eV"]
    P = {f: rows[:, j][:, None] for j, f in enumerate(("lnTe", "Y", "Npar", "N2"))}
    P["X"] = np.full((len(rows), 1), 0.3)
    a = _alpha(H, P, slice(None), om, mode, 1, 0.0)
    assert (a[rows[:, 0] > LN20 + 1e-12] > 0).all() and not _flags(H, P)[rows[:, 0] > LN20 + 1e-12].any()


def test_zero_box_refuses_non_finite_inputs(H):
    """A NaN or +-inf in any one input, at any position in the box, clears the
    flag: boxes of 1, 8 and 240 points that are flagged without it, cold (all
    Te < 20 eV) and warm (both harmonics exact zeros)."""
    rng = np.random.default_rng(11)
    for base in ((np.log(5.0), 0.4, 0.3, 0.6), (np.log(40.0), 1.4, 0.3, 0.6)):
        for k in (1, 8, 240):
            pos = range(k) if k <= 8 else (0, 1, 2, 119, 120, 237, 238, 239)
            cases = [(p, j, v) for p in pos for j in range(4) for v in (np.nan, np.inf, -np.inf)]
            n = len(cases)
            P = {f: base[j] * (1 + 1e-3 * rng.uniform(-1, 1, (n, k))) for j, f in enumerate(("lnTe", "Y", "Npar", "N2"))}
            assert _flags(H, P).all(), (base, k)
            for i, (p, j, v) in enumerate(cases):
                P[("lnTe", "Y", "Npar", "N2")[j]][i, p] = v
            fl = _flags(H, P)
            assert not fl.any(), (base, k, [cases[i] for i in np.flatnonzero(fl)[:5]])


@pytest.mark.parametrize("mode", [1, -1])
def test_zero_box_sound_at_extreme_inputs(H, mode):
    """Finite inputs far outside any plasma, on a grid: Y from 1e-199 to 1e199,
    ln Te up to 699, |N_par| up to 0.9999, with N_perp^2 in the sweep's range.
    Either the flag refuses or alpha is a zero in all three variants (Y >= 1e150
    once gave a set flag where r^2 overflows and the body returns NaN)."""
    om = 2 * np.pi * 92.5e9
    rows = np.array([(lte, Y, npar, npar * npar + nperp2)
                     for lte in (np.log(40.0), np.log(3e4), 20.0, 100.0, 299.0, 301.0, 360.0, 370.0, 500.0, 699.0)
                     for Y in (1e-199, 1e-150, 1e-101, 1e-99, 1e-10, 0.1, 1.4, 10.0, 1e10, 1e99, 1e101, 1e150,
                               1e153, 1e154, 1e155, 1e199)
                     for npar in (0.0, 0.3, -0.9, 0.9999) for nperp2 in (1e-6, 1e-3, 0.5, 1.2)])
    P = {f: rows[:, j][:, None].copy() for j, f in enumerate(("lnTe", "Y", "Npar", "N2"))}
    P["X"] = np.full((len(rows), 1), 0.3)
    fl = _flags(H, P)
    print(f"mode {mode:+d} extremes: {len(rows)} points, {int(fl.sum())} flagged")
    assert fl.sum() > 100
    _assert_zero(H, P, fl, om, mode, "extremes")


@pytest.fixture(scope="module")
def stage_points():
    from test_warm_host import _stage_points

    return _stage_points()


def test_zero_box_fires_on_stage_point_runs(H, stage_points):
    """The flag fires on runs of consecutive points along the rays of
    test_warm_host._stage_points() (24 rays of the headline fan, a state every 50
    steps): the share of runs of 2 and of 4 flagged, above 0, and sound there."""
    n_rays = 24
    pts = stage_points.reshape(-1, n_rays, 6)  # (sample, ray, (omega, X, Y, |N|, N_par, Te))
    om = float(pts[0, 0, 0])
    for run in (2, 4):
        rows = np.array([pts[s:s + run, r] for r in range(n_rays) for s in range(pts.shape[0] - run + 1)])
        P = dict(lnTe=np.log(rows[:, :, 5]), Y=rows[:, :, 2], Npar=rows[:, :, 4], N2=rows[:, :, 3] ** 2,
                 X=rows[:, :, 1])
        fl = _flags(H, P)
        warm = fl & (P["lnTe"].max(1) >= LN20)
        print(f"stage-point runs of {run}: {len(fl)} runs, flagged {fl.mean():.3f}, flagged and warm {warm.mean():.3f}")
        assert fl.mean() > 0
        _assert_zero(H, P, fl, om, 1, f"stage-point runs of {run}")


@pytest.mark.parametrize("f", [28e9, 92.5e9, 140e9])
@pytest.mark.parametrize("mode", [1, -1])
def test_tiny_alpha_skip_bounded_pointwise(H, mode, f):
    """alpha with tiny_alpha 1e-20 and 1e-12 against tiny_alpha 0 over
    test_h3_fast_host's random tuples and edge cases: the same finite / NaN
    pattern, |alpha(tiny) - alpha(0)| <= 2 tiny (two harmonics can be skipped)
    + 4e-16 |alpha(0)| (the rounding of the sums the skipped terms left, as
    test_tiny_alpha_skip_bounded), and the skip fires: some alpha move."""
    om = 2 * np.pi * f
    pts = np.vstack([_random(seed=7 + mode), _edges()])
    cols = [np.ascontiguousarray(pts[:, j]) for j in (1, 2, 3, 4, 5)]

    def alpha(tiny):
        out = np.full(len(pts), np.nan)
        with np.errstate(all="ignore"):
            H.sp_alpha_pts(len(pts), *[_p(c) for c in cols], om, mode, tiny, _p(out))
        return out

    a0 = alpha(0.0)
    for tiny in (1e-20, 1e-12):
        a = alpha(tiny)
        assert np.array_equal(np.isfinite(a), np.isfinite(a0)) and np.array_equal(np.isnan(a), np.isnan(a0))
        fin = np.isfinite(a0)
        d = np.abs(a[fin] - a0[fin])
        moved = d > 0
        print(f"{f / 1e9:g} GHz mode {mode:+d} tiny {tiny:g}: {int(fin.sum())} finite of {len(pts)}, "
              f"{moved.mean():.4f} moved, max |d alpha| / tiny {d.max() / tiny:.4g}, "
              f"max (|d alpha| - 4e-16 |alpha|) / tiny {(d - 4e-16 * np.abs(a0[fin])).max() / tiny:.4g}")
        bad = d > 2 * tiny + 4e-16 * np.abs(a0[fin])
        assert not bad.any(), (pts[fin][bad][:5], a[fin][bad][:5], a0[fin][bad][:5])
        assert moved.any()
