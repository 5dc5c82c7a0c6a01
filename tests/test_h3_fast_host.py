"""Harmonic 3 dismissed from the prologue's outputs (torj_math.hpp
h3_fast_negligible, GLTable::h3_fast), host build, on CPU: wherever the cheap
test says "negligible" albajar_harmonic<3> itself returns a zero and alpha is
bit-identical with the switch on and off; its bounds dominate the ones they
replace (U 2^(ceil(y_ub) + 1) >= B0 E_max, y_ub >= ymax); and it fires on the
headline fan's stage points."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
OM = 2 * np.pi * 92.5e9


@pytest.fixture(scope="module")
def H():
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", "libh3_fast_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # libwarm_host.so's flags (tests/native/Makefile), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "h3_fast_host.hip")])
    L = C.CDLL(out)
    L.hf_setup.argtypes = [C.c_int, _dp, _dp]
    L.hf_eval.argtypes = [C.c_int] + [_dp] * 6 + [C.c_int, C.c_double, _dp, _dp, _ip, _ip, _dp, _dp, _dp, _dp, _ip]
    t, w = np.polynomial.legendre.leggauss(24)
    L.hf_setup(24, np.ascontiguousarray(t).ctypes.data_as(_dp), np.ascontiguousarray(w).ctypes.data_as(_dp))
    return L


def _eval(H, pts, mode, tiny):
    """hf_eval over rows (omega, X, Y, |N|, N_par, Te) -> dict of per-point arrays"""
    pts = np.asarray(pts, dtype=float)
    n = len(pts)
    cols = [np.ascontiguousarray(pts[:, k]) for k in range(6)]
    d = {k: np.zeros(n) for k in ("on", "off", "bound", "y_ub", "b0e", "ymax")}
    i = {k: np.zeros(n, dtype=np.int32) for k in ("reach", "verdict", "outcome")}
    H.hf_eval(n, *[c.ctypes.data_as(_dp) for c in cols], mode, tiny, d["on"].ctypes.data_as(_dp),
              d["off"].ctypes.data_as(_dp), i["reach"].ctypes.data_as(_ip), i["verdict"].ctypes.data_as(_ip),
              d["bound"].ctypes.data_as(_dp), d["y_ub"].ctypes.data_as(_dp), d["b0e"].ctypes.data_as(_dp),
              d["ymax"].ctypes.data_as(_dp), i["outcome"].ctypes.data_as(_ip))
    d.update(i)
    return d


@pytest.fixture(scope="module")
def stage_points():
    from test_warm_host import _stage_points

    return _stage_points()


def _golden(mode):
    g = np.array(json.load(open(os.path.join(HERE, "golden", "albajar.json")))["rows"], dtype=float)
    return g[g[:, 6] == mode][:, :6]


def _random(n=200000, seed=7):
    """Te 20 eV - 30 keV log-uniform, Y 0.2 - 1.2, |N_par| <= 0.98, X 0 - 0.999,
    |N| in the dispersion-free range 0.05 - 1.2"""
    r = np.random.default_rng(seed)
    return np.column_stack([np.full(n, OM), r.uniform(0.0, 0.999, n), r.uniform(0.2, 1.2, n),
                            r.uniform(0.05, 1.2, n), r.uniform(-0.98, 0.98, n),
                            np.exp(r.uniform(np.log(20.0), np.log(3e4), n))])


def _ulps(x, ks):
    out = []
    for k in ks:
        v = x
        for _ in range(abs(k)):
            v = np.nextafter(v, np.inf if k > 0 else -np.inf)
        out.append(float(v))
    return out


def _edges():
    """N_perp = 0, N_par^2 >= 1, X >= 1, Y a few ulp either side of sqrt(1 - N_par^2) / 3
    and / 2, Te = 20 either side, NaN and +-inf in each input in turn"""
    bases = [(OM, 0.3, 0.40, 0.8, 0.3, 5e3),   # harmonic 3 alone, warm
             (OM, 0.3, 0.55, 0.8, 0.3, 5e3),   # beside harmonic 2
             (OM, 0.3, 0.40, 0.8, 0.3, 100.0),  # cold: exact zeros
             (OM, 0.6, 0.34, 0.5, -0.2, 2e4)]
    rows = []
    for b in bases:
        om, X, Y, N, Npar, Te = b
        rows.append(b)
        rows.append((om, X, Y, abs(Npar), Npar, Te))                    # N_perp = 0
        rows.append((om, X, Y, np.nextafter(abs(Npar), 1.0), Npar, Te))  # N_perp tiny
        for npar in (1.0, -1.0, 1.2, np.nextafter(1.0, 0.0)):
            rows.append((om, X, Y, 1.5, npar, Te))                       # N_par^2 >= 1 and just below
        for x in (1.0, np.nextafter(1.0, 0.0), 1.5):
            rows.append((om, x, Y, N, Npar, Te))
        sq = np.sqrt(1.0 - Npar * Npar)
        for m in (3.0, 2.0):
            for y in _ulps(sq / m, range(-4, 5)):
                rows.append((om, X, y, N, Npar, Te))
        for te in _ulps(20.0, (-2, -1, 0, 1, 2)):
            rows.append((om, X, Y, N, Npar, te))
        for k in range(6):
            for v in (np.nan, np.inf, -np.inf):
                r = list(b)
                r[k] = v
                rows.append(tuple(r))
        for v in (0.0, -0.0, 1e-300, 1e300):                             # zeros and extremes of Y, |N|, Te
            for k in (2, 3, 5):
                r = list(b)
                r[k] = v
                rows.append(tuple(r))
    return np.array(rows, dtype=float)


def _point_sets(stage_points):
    yield "stage", stage_points, 1
    for mode in (1, -1):
        yield f"golden{mode:+d}", _golden(mode), mode
        yield f"random{mode:+d}", _random(seed=7 + mode), mode
        yield f"edges{mode:+d}", _edges(), mode


def _bits(a):
    return (a + 0.0).view(np.int64)  # zeros compared as zeros


@pytest.mark.parametrize("tiny", [1e-20, 0.0])
def test_soundness_and_dominance(H, stage_points, tiny):
    """Soundness: verdict true => albajar_harmonic<3> returns a zero there (exact
    zero or skipped as negligible) and alpha is bit-identical with the switch on
    and off.  Dominance: where harmonic 3 is present, U 2^(ceil(y_ub) + 1) >= B0 E_max
    and y_ub >= ymax (a refusal reports infinite bounds; non-finite values are
    excluded only when both sides are)."""
    n_true = 0
    for name, pts, mode in _point_sets(stage_points):
        with np.errstate(all="ignore"):
            d = _eval(H, pts, mode, tiny)
        v = d["verdict"] == 1
        print(f"{name} tiny {tiny:g}: {len(pts)} points, {int(d['reach'].sum())} reach harmonic 3, "
              f"verdict true on {int(v.sum())}; outcomes integrated/zero/negligible "
              f"{[int((d['outcome'][d['reach'] == 1] == k).sum()) for k in (0, 1, 2)]}")
        assert np.all(d["reach"][v] == 1)
        assert np.all(np.isin(d["outcome"][v], (1, 2))), (name, pts[v & ~np.isin(d["outcome"], (1, 2))][:5])
        nan = np.isnan(d["off"])
        assert np.array_equal(np.isnan(d["on"]), nan), name
        assert np.array_equal(_bits(d["on"][~nan]), _bits(d["off"][~nan])), name
        r = d["reach"] == 1
        for hi, lo in (("bound", "b0e"), ("y_ub", "ymax")):
            a, b = d[hi][r], d[lo][r]
            both = ~np.isfinite(a) & ~np.isfinite(b)
            bad = ~both & ~(a >= b)
            assert not bad.any(), (name, hi, pts[r][bad][:5], a[bad][:5], b[bad][:5])
        n_true += int(v.sum())
    assert n_true > 0


def test_fires_on_the_fan(H, stage_points):
    """With tiny_alpha = 1e-20 the verdict is true on at least 95 % of the
    harmonic-3 integrals of the fan's stage points that albajar_harmonic<3> skips;
    without it (the rel form beside harmonic 2, and the exact zeros) on some."""
    d = _eval(H, stage_points, 1, 1e-20)
    skipped = (d["reach"] == 1) & (d["outcome"] == 2)
    share = (d["verdict"][skipped] == 1).mean()
    zeros = (d["reach"] == 1) & (d["outcome"] == 1)
    fin = skipped & (d["verdict"] == 1) & (d["bound"] > 0) & (d["b0e"] > 0)
    slack = np.log2(d["bound"][fin] / d["b0e"][fin]) if fin.any() else np.zeros(1)
    print(f"tiny 1e-20: {int(skipped.sum())} skipped integrals, verdict true on {share:.4f}; "
          f"{int(zeros.sum())} exact zeros, verdict true on {(d['verdict'][zeros] == 1).mean():.4f}; "
          f"log2(bound / B0 E_max) median {np.median(slack):.1f} max {slack.max():.1f}")
    assert skipped.sum() > 100 and share >= 0.95
    e = _eval(H, stage_points, 1, 0.0)
    dismissible = (e["reach"] == 1) & (e["outcome"] != 0)
    share0 = (e["verdict"][dismissible] == 1).mean()
    print(f"tiny 0: {int(dismissible.sum())} zero or skipped integrals, verdict true on {share0:.4f}")
    assert share0 > 0
