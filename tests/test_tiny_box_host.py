"""The block tiny box on CPU (torj_math.hpp TBox, tiny_box_add, tiny_box_flag),
in both forms of the node exponent (TORJ_NODE_GAMMA_LIN 1, the default, and 0):
a set flag means abs_albajar_fast_body, with negl_skip on and the same
tiny_alpha, returns a zero of either sign, never NaN, at every point the ray's
two boxes cover -- and there |alpha(tiny_alpha = 0)| <= 2 tiny_alpha, the promise
the tiny skip makes, with the h3_fast shortcut on and off.  The trajectory
kernel writes "zero_box_flag or tiny_box_flag"; its dead-box latch needs the
disjunction monotone.

Host build of tests/native/tiny_box_host.hip (the device takes v_max_f64 /
v_min_f64 / v_max_f32 where the host takes fmax / fmin / fmaxf; non-finite
inputs are the zero box's chk word's business in both)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_skip_proofs_host import _boxes, _eps
from test_zbox_latch_host import CADENCES, STRIDE

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
FIELDS = ("lnTe", "Y", "Npar", "N2", "X")
OM = 2 * np.pi * 92.5e9
# boxes per (mode, frequency, tiny_alpha): single points, 8-point boxes, whole 60-step blocks
K_SHARE = ((1, 24000), (8, 33000), (240, 3000))
N_BOXES = sum(n for _, n in K_SHARE)
# Floors on the boxes tiny_box_flag sets among N_BOXES, per mode: half the share
# measured (mode +1: 0.0074 - 0.0076 at every frequency, both tiny_alpha and both
# forms, 0.0013 beyond zero_box_flag; mode -1: 0.0002, where den keeps one sign
# over few boxes), so that the sweep cannot pass empty
FIRE_FLOOR = {1: int(0.5 * 0.0074 * N_BOXES), -1: 5}
# a point the flag fires on in both modes: harmonic 2 absent, harmonic 3 far below its resonance
BASE = dict(lnTe=np.log(500.0), Y=0.42, Npar=1e-3, N2=0.8, X=0.3)


def _p(a):
    return a.ctypes.data_as(_dp)


def _pi(a):
    return a.ctypes.data_as(_ip)


@pytest.fixture(scope="module", params=[1, 0], ids=["gamma_lin1", "gamma_lin0"])
def H(request):
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", f"libtiny_box_host{request.param}.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # libwarm_host.so's flags (tests/native/Makefile), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           f"-DTORJ_NODE_GAMMA_LIN={request.param}",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "tiny_box_host.hip")])
    L = C.CDLL(out)
    L.tb_setup.argtypes = [C.c_int, _dp, _dp]
    L.tb_flags.argtypes = [C.c_int, C.c_int] + [_dp] * 5 + [C.c_double, C.c_int, C.c_double, _ip, _ip]
    L.tb_alpha.argtypes = [C.c_int] + [_dp] * 5 + [C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, _dp]
    L.tb_prefix.argtypes = [C.c_int, C.c_int] + [_dp] * 5 + [C.c_double, C.c_int, C.c_double] + [_ip] * 4
    L.tb_latched.argtypes = ([C.c_int] * 5 + [_ip, _ip] + [_dp] * 5 + [C.c_double, C.c_int, C.c_double] +
                             [_ip, _ip])
    assert L.tb_gamma_lin() == request.param
    t, w = np.polynomial.legendre.leggauss(24)
    L.tb_setup(24, _p(np.ascontiguousarray(t)), _p(np.ascontiguousarray(w)))
    return L


def _cols(P, sel=slice(None)):
    return [np.ascontiguousarray(P[f][sel], dtype=float) for f in FIELDS]


def _flags(H, P, om, mode, tiny):
    """P: dict of (nb, k) arrays -> (zero_box_flag, tiny_box_flag) per box"""
    nb, k = P["lnTe"].shape
    z, t = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    H.tb_flags(nb, k, *[_p(c) for c in _cols(P)], om, mode, tiny, _pi(z), _pi(t))
    return z == 1, t == 1


def _alpha(H, P, sel, om, mode, negl, h3, tiny):
    cols = [c.ravel() for c in _cols(P, sel)]
    out = np.full(len(cols[0]), np.nan)
    with np.errstate(all="ignore"):
        H.tb_alpha(len(out), *[_p(np.ascontiguousarray(c)) for c in cols], om, mode, negl, h3, tiny, _p(out))
    return out


def _assert_sound(H, P, sel, om, mode, tiny, what):
    """at every point of the boxes sel: alpha(tiny) is a zero, and the exact leg's
    alpha is within the skip's promise, h3_fast on and off"""
    if not np.any(sel):
        return
    for h3 in (1, 0):
        a = _alpha(H, P, sel, om, mode, 1, h3, tiny)
        bad = ~(a == 0.0)
        if bad.any():
            i = np.flatnonzero(bad)[:3]
            rows = {f: P[f][sel].ravel()[i] for f in FIELDS}
            raise AssertionError(f"{what}: flag set, alpha {a[i]} (h3_fast {h3}, tiny {tiny:g}) at {rows}")
        a0 = _alpha(H, P, sel, om, mode, 1, h3, 0.0)
        bad = ~(np.abs(a0) <= 2 * tiny)
        assert not bad.any(), (what, h3, a0[bad][:3])


def _boxes_x(nb, k, rng):
    """test_skip_proofs_host._boxes with X as the other inputs are drawn: around a
    centre in (0, 1.2), relative widths log-uniform 1e-12 - 0.3, and the fresh
    points' X inside the range the added points span"""
    P, F = _boxes(nb, k, rng)
    c = rng.uniform(0.0, 1.2, nb)
    wd = np.exp(rng.uniform(np.log(1e-12), np.log(0.3), nb))
    P["X"] = c[:, None] * (1.0 + wd[:, None] * rng.uniform(-1.0, 1.0, (nb, k)))
    lo, hi = P["X"].min(1)[:, None], P["X"].max(1)[:, None]
    F["X"] = np.clip(lo + (hi - lo) * rng.uniform(0.0, 1.0, (nb, k)), lo, hi)
    return P, F


@pytest.fixture(scope="module")
def boxes():
    """the random boxes of the soundness sweep, made once for every parameter"""
    rng = np.random.default_rng(1811)
    return [(k,) + _boxes_x(nb, k, rng) for k, nb in K_SHARE]


@pytest.mark.parametrize("f", [28e9, 92.5e9, 140e9])
@pytest.mark.parametrize("tiny", [1e-20, 1e-12])
@pytest.mark.parametrize("mode", [1, -1])
def test_tiny_box_sound_on_random_boxes(H, boxes, mode, tiny, f):
    """Soundness: tiny_box_flag => alpha(tiny_alpha) == 0 (either sign), not NaN, and
    |alpha(0)| <= 2 tiny_alpha, h3_fast on and off, at every added point and at as many
    fresh points of the box's ranges, X included; never set with tiny_alpha 0; and at
    least FIRE_FLOOR boxes fire."""
    om = 2 * np.pi * f
    n_fire = n_new = 0
    for k, P, F in boxes:
        z, t = _flags(H, P, om, mode, tiny)
        _, t0 = _flags(H, P, om, mode, 0.0)
        assert not t0.any(), "flag set with tiny_alpha 0"
        _assert_sound(H, P, t, om, mode, tiny, f"k {k} added points")
        _assert_sound(H, F, t, om, mode, tiny, f"k {k} fresh points")
        n_fire += int(t.sum())
        n_new += int((t & ~z).sum())
    print(f"mode {mode:+d} {f / 1e9:g} GHz tiny {tiny:g}: tiny_box_flag on {n_fire / N_BOXES:.4f} of {N_BOXES} "
          f"boxes, {n_new / N_BOXES:.4f} beyond zero_box_flag")
    assert n_fire >= FIRE_FLOOR[mode], (n_fire, FIRE_FLOOR[mode])


def _one(**kw):
    return {f: np.array([[float(kw.get(f, BASE[f]))]]) for f in FIELDS}


def _rows(rows):
    """list of dicts of overrides of BASE -> single-point boxes"""
    return {f: np.array([[float(r.get(f, BASE[f]))] for r in rows]) for f in FIELDS}


def _prologue(P, mode):
    """D, Nt^2 and den of albajar_prologue at every point (numpy, for building cases)"""
    X, Y = P["X"], P["Y"]
    c2 = P["Npar"] ** 2 / P["N2"]
    s2 = 1 - c2
    rho = np.sqrt(Y ** 2 * s2 ** 2 + 4 * (1 - X) ** 2 * c2)
    D = 2 * (1 - X) - Y ** 2 * s2 - mode * Y * rho
    with np.errstate(all="ignore"):
        nt2 = 1 - X * 2 * (1 - X) / D
    return D, nt2, (1 - X) - nt2 * s2


@pytest.mark.parametrize("mode", [1, -1])
def test_tiny_box_refusals(H, mode):
    """The base point fires; a NaN or +-inf in any input at any position, X >= 1,
    X = 0, D <= 0 and a box over which den's interval straddles 0 are refused."""
    for tiny in (1e-20, 1e-12):
        z, t = _flags(H, _one(), OM, mode, tiny)
        assert t[0] and not z[0]
        _assert_sound(H, _one(), t, OM, mode, tiny, "base")
    rng = np.random.default_rng(3)
    for k in (1, 8, 240):
        pos = range(k) if k <= 8 else (0, 1, 119, 238, 239)
        cases = [(p, j, v) for p in pos for j in range(5) for v in (np.nan, np.inf, -np.inf)]
        n = len(cases)
        P = {f: BASE[f] * (1 + 1e-3 * rng.uniform(-1, 1, (n, k))) for f in FIELDS}
        assert _flags(H, P, OM, mode, 1e-20)[1].all()
        for i, (p, j, v) in enumerate(cases):
            P[FIELDS[j]][i, p] = v
        z, t = _flags(H, P, OM, mode, 1e-20)
        assert not t.any() and not z.any(), [cases[i] for i in np.flatnonzero(t | z)[:5]]
    # X >= 1, X = 0 and below the flag's own floor, alone and beside a base point
    for x in (1.0, 1.0 + 1e-12, 1.2, 0.0, 1e-13, -0.1, np.nextafter(1.0, 0.0)):
        for P in (_one(X=x), {f: np.array([[BASE[f], _one(X=x)[f][0, 0]]]) for f in FIELDS}):
            assert not _flags(H, P, OM, mode, 1e-20)[1].any(), x
    # D <= 0: beyond the mode's cut-off / resonance in X, on a grid
    g = [dict(X=x, Y=y, Npar=n) for x in np.linspace(0.05, 0.999, 400) for y in (0.36, 0.42, 0.48)
         for n in (0.0, 0.1, 0.3)]
    P = _rows(g)
    D, nt2, den = _prologue(P, mode)
    t = _flags(H, P, OM, mode, 1e-20)[1]
    assert not t[(D <= 0).ravel()].any() and not t[~(nt2 > 0).ravel()].any()
    print(f"mode {mode:+d}: X grid, {int(t.sum())} of {len(t)} flagged, {(D <= 0).sum()} with D <= 0, "
          f"{(~(nt2 > 0)).sum()} with Nt^2 <= 0")
    assert t.any() and (mode < 0 or (D <= 0).any())
    _assert_sound(H, P, t, OM, mode, 1e-20, "X grid")
    # den's interval straddling 0.  At real points with Y < 1 den > 0 in either mode, but
    # the box knows only c2 <= its maximum, so its lower bound on den is that of s2 = 1,
    # X_lo f_lo - X_hi: an oblique box (c2 >= 1e-5) whose X spans more than the factor f
    # is refused though each of its points alone fires (mode +1; in mode -1, f <= 1, no
    # oblique box passes), and the same box turned quasi-perpendicular, where the
    # prologue has no den, fires in both modes
    pair = lambda npar: {f: np.array([[_one(X=0.2, Npar=npar)[f][0, 0], _one(X=0.3, Npar=npar)[f][0, 0]]])
                         for f in FIELDS}
    D, nt2, den = _prologue(pair(0.1), mode)
    assert (D > 0).all() and (nt2 > 0).all() and (den > 0).all()
    alone = [_flags(H, _one(X=x, Npar=0.1), OM, mode, 1e-20)[1][0] for x in (0.2, 0.3)]
    assert alone == [mode > 0] * 2, alone
    assert not _flags(H, pair(0.1), OM, mode, 1e-20)[1][0]
    t = _flags(H, pair(1e-3), OM, mode, 1e-20)[1]
    assert t[0]
    _assert_sound(H, pair(1e-3), t, OM, mode, 1e-20, "quasi-perpendicular pair")


def _lines():
    """name -> (field or 'tiny', values from inside the fired region outwards): one
    line through BASE per inequality of tiny_box_flag"""
    geo = lambda a, b, n=400: np.exp(np.linspace(np.log(a), np.log(b), n))
    return {
        "X -> 1 (X < 1, D, Nt^2)": ("X", np.linspace(BASE["X"], 1.0, 400)),
        "X -> 0 (den, X > 1e-12)": ("X", geo(BASE["X"], 1e-14)),
        "Y down (G > 1)": ("Y", np.linspace(BASE["Y"], 0.3, 400)),
        "Y up (harmonic 2 present)": ("Y", np.linspace(BASE["Y"], 0.6, 400)),
        "Te up (the bound itself)": ("lnTe", np.linspace(BASE["lnTe"], np.log(3e4), 400)),
        "|N_par| up (G > 1, harmonic 2)": ("Npar", np.linspace(BASE["Npar"], 0.9, 400)),
        "N_par down (c2 = 1e-5)": ("Npar", geo(BASE["Npar"], 1e-5)),
        "N_perp^2 down (s2)": ("N2", BASE["Npar"] ** 2 + geo(BASE["N2"] - BASE["Npar"] ** 2, 1e-14)),
        "|N|^2 up": ("N2", geo(BASE["N2"], 1e8)),
        "tiny_alpha down": ("tiny", geo(1e-12, 1e-300)),
    }


@pytest.mark.parametrize("mode", [1, -1])
def test_tiny_box_sound_at_its_thresholds(H, mode):
    """Along a line through the base point per inequality of the flag (X -> 1 and
    X -> 0, Y down to G = 1 and up to harmonic 2, Te up to where the bound fails,
    |N_par| up and down across the quasi-perpendicular switch, N_perp^2 -> 0,
    |N|^2 up, tiny_alpha down): every place the flag flips is bracketed to an
    ulp-scale interval by bisection and then approached from both sides at the
    offsets of test_skip_proofs_host._eps (+-4 ulp .. +-1e-8 relative); the flag
    is sound on both sides and is seen set and clear.  Lines that cross no
    threshold (the quasi-perpendicular switch changes no flag) are sound along
    their whole length."""
    e = _eps()
    crossed = 0
    for name, (field, vals) in _lines().items():
        def flag(v):
            v = np.atleast_1d(v)
            if field == "tiny":
                return np.array([_flags(H, _one(), OM, mode, x)[1][0] for x in v])
            return _flags(H, _rows([{field: x} for x in v]), OM, mode, 1e-20)[1]

        fl = flag(vals)
        if field != "tiny":
            _assert_sound(H, _rows([{field: x} for x in vals]), fl, OM, mode, 1e-20, name)
        flips = np.flatnonzero(fl[1:] != fl[:-1])
        print(f"mode {mode:+d} {name}: {int(fl.sum())} of {len(fl)} flagged, {len(flips)} flips")
        assert fl[0], name
        for i in flips:
            a, b = vals[i], vals[i + 1]
            fa = fl[i]
            for _ in range(80):
                mid = 0.5 * (a + b) if field != "tiny" else np.sqrt(a * b)
                if mid == a or mid == b:
                    break
                if flag(mid)[0] == fa:
                    a = mid
                else:
                    b = mid
            near = a * (1 + e)
            fn = flag(near)
            assert fn.any() and not fn.all(), (name, a, fn)
            if field == "tiny":
                for x, f1 in zip(near, fn):
                    _assert_sound(H, _one(), np.array([f1]), OM, mode, x, name)
            else:
                _assert_sound(H, _rows([{field: x} for x in near]), fn, OM, mode, 1e-20, name)
            crossed += 1
    assert crossed >= 8, crossed


def _walks(nb, k, rng):
    """random walks from centres in and around the region the tiny flag fires in
    (harmonic 2 absent, 3 Y near 1 + |N_par|, X inside (0, 1)): a drift plus
    jitter per input, relative sizes log-uniform 1e-12 - 0.3 per sequence"""
    npar = rng.uniform(-0.5, 0.5, nb) * rng.choice([1.0, 1e-3], nb)  # half of them quasi-perpendicular
    c = dict(Te=np.exp(rng.uniform(np.log(10.0), np.log(5e3), nb)),
             Y=(1 + np.abs(npar)) / 3 * rng.uniform(0.9, 1.5, nb), Npar=npar,
             Np2=np.exp(rng.uniform(np.log(1e-3), np.log(1.2), nb)), X=rng.uniform(0.0, 1.05, nb))
    v = {}
    for f in c:
        drift = np.exp(rng.uniform(np.log(1e-12), np.log(0.3), nb)) * rng.choice([-1.0, 1.0], nb)
        jit = np.exp(rng.uniform(np.log(1e-12), np.log(0.3), nb))
        t = np.linspace(0.0, 1.0, k)[None, :]
        v[f] = c[f][:, None] * (1.0 + drift[:, None] * t + jit[:, None] * rng.uniform(-1.0, 1.0, (nb, k)))
    with np.errstate(all="ignore"):
        P = dict(lnTe=np.log(v["Te"]), Y=v["Y"], Npar=v["Npar"], N2=v["Npar"] ** 2 + v["Np2"], X=v["X"])
    bad = np.flatnonzero(rng.uniform(size=nb) < 0.05)  # a non-finite input in one place
    for b in bad:
        P[FIELDS[rng.integers(0, 5)]][b, rng.integers(0, k)] = (np.nan, np.inf, -np.inf)[rng.integers(0, 3)]
    return {f: np.ascontiguousarray(P[f]) for f in FIELDS}


@pytest.fixture(scope="module")
def seqs():
    rng = np.random.default_rng(4711)
    return [_walks(nb, k, rng) for k, nb in ((8, 50000), (24, 45000), (240, 5000))]


@pytest.mark.parametrize("mode", [1, -1])
def test_either_flag_false_stays_false(H, seqs, mode):
    """tests/test_zbox_latch_host.py's sweep over "zero_box_flag or tiny_box_flag":
    no sequence has a prefix with a false flag before a longer one with a true
    flag; the sweep is live (flags going false mid-sequence, staying true, false
    from the first point, and true by the tiny flag alone, thousands of each)."""
    n_mid = n_true = n_first = n_tiny = 0
    for P in seqs:
        nb, k = P["lnTe"].shape
        fin, ff, back, ts = (np.zeros(nb, dtype=np.int32) for _ in range(4))
        H.tb_prefix(nb, k, *[_p(P[f]) for f in FIELDS], OM, mode, 1e-20, _pi(fin), _pi(ff), _pi(back), _pi(ts))
        bad = np.flatnonzero(back > 0)
        assert bad.size == 0, (f"flag false after {ff[bad[0]]} points, true again after {back[bad[0]]}",
                               {f: P[f][bad[0]][:back[bad[0]]] for f in FIELDS})
        n_mid += int((ff > 1).sum())
        n_true += int(fin.sum())
        n_first += int((ff == 1).sum())
        n_tiny += int(ts.sum())
        print(f"mode {mode:+d} k {k}: true to the end {fin.mean():.3f}, false from the first point "
              f"{(ff == 1).mean():.3f}, going false later {(ff > 1).mean():.3f}, tiny alone at some prefix {ts.mean():.3f}")
    assert n_mid >= 2000 and n_true >= 2000 and n_first >= 10000 and n_tiny >= 2000, (n_mid, n_true, n_first, n_tiny)


def test_latched_flags_equal_unlatched(H, seqs):
    """traj_run's latched bookkeeping over both boxes writes the unlatched flags
    (tests/test_zbox_latch_host.py test_latched_flags_equal_unlatched, with the
    vote and the final flag over the disjunction); the latch is seen to fire."""
    rng = np.random.default_rng(78)
    fired = 0
    for P in seqs:
        nb, k = P["lnTe"].shape
        trips = k // STRIDE
        for length in (np.full(nb, trips, dtype=np.int32), rng.integers(1, trips + 1, nb).astype(np.int32)):
            idx = np.minimum(np.arange(k)[None, :], (length * STRIDE - 1)[:, None])
            Q = {f: np.ascontiguousarray(np.take_along_axis(P[f], idx, 1)) for f in FIELDS}
            ref, junk = np.zeros(nb, dtype=np.int32), [np.zeros(nb, dtype=np.int32) for _ in range(3)]
            H.tb_prefix(nb, k, *[_p(Q[f]) for f in FIELDS], OM, 1, 1e-20, _pi(ref), *[_pi(j) for j in junk])
            for wave in (1, 64):
                for cad in CADENCES:
                    cd = np.ascontiguousarray([c for c in cad if c <= trips], dtype=np.int32)
                    got, lat = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
                    H.tb_latched(nb, k, STRIDE, wave, len(cd), _pi(cd), _pi(length), *[_p(P[f]) for f in FIELDS],
                                 OM, 1, 1e-20, _pi(got), _pi(lat))
                    assert np.array_equal(got, ref), (wave, cad, np.flatnonzero(got != ref)[:5])
                    assert not ((got == 1) & (lat > 0)).any()
                    fired += int((lat > 0).sum()) if len(cad) else 0
    print(f"{fired} boxes latched over all cadences")
    assert fired > 50000


@pytest.fixture(scope="module")
def stage_points():
    from test_warm_host import _stage_points

    return _stage_points(24, 20)


def test_tiny_box_fires_on_the_headline_fan(H, stage_points):
    """24 rays of the headline fan, every 20th step of the oracle's trace, for
    every ray the non-overlapping boxes of four consecutive samples (60 steps).
    Among the boxes zero_box_flag leaves false, those whose every point has
    alpha(tiny_alpha = 1e-20) == 0: tiny_box_flag fires on at least 90 % of them,
    and on no box that holds a point with alpha != 0."""
    n_rays = 24
    pts = stage_points.reshape(-1, n_rays, 6)  # (sample, ray, (omega, X, Y, |N|, N_par, Te))
    om = float(pts[0, 0, 0])
    rows = np.array([pts[s:s + 4, r] for r in range(n_rays) for s in range(0, pts.shape[0] - 3, 4)])
    P = dict(lnTe=np.log(rows[:, :, 5]), Y=rows[:, :, 2], Npar=rows[:, :, 4], N2=rows[:, :, 3] ** 2, X=rows[:, :, 1])
    z, t = _flags(H, P, om, 1, 1e-20)
    a = _alpha(H, P, slice(None), om, 1, 1, 1, 1e-20).reshape(len(rows), 4)
    zero = (a == 0.0).all(1)
    want = ~z & zero
    print(f"{len(rows)} boxes: zero_box_flag {int(z.sum())}, all-zero and unflagged {int(want.sum())}, "
          f"tiny_box_flag on {int((t & want).sum())} of them, {int((t & ~zero).sum())} on boxes with alpha != 0")
    assert want.sum() > 100
    assert not (t & ~zero).any()
    assert (t & want).sum() >= 0.9 * want.sum(), ((t & want).sum(), want.sum())
    _assert_sound(H, P, t, om, 1, 1e-20, "stage-point boxes")
