"""The double-double record function of the device-built cell table
(torj_celltab.hpp cell_record, what k_cell_table runs per (cell, field)) on CPU,
against the exact value of every entry

    A_ji = (sum_b sum_a M_jb M_ia c_ba) / 36 / hR^i / hZ^j,    M = 6 B,

computed with fractions.Fraction from the double inputs (B: bweights' power basis).

Bars (derived, not measured).  With S = sum |M_jb M_ia c_ba| / (36 hR^i hZ^j):
* cell_record: |got - exact| <= 1 ulp(exact) + 2^-80 S.  The products M M c are exact
  double-doubles; 15 double-double sums, the division by 36 and up to six by hR, hZ
  each err by a few 2^-104 of a value no larger than S, together below 2^-97 S; the
  one rounding to double adds half an ulp.  Double-double carries >= 100 bits, so the
  bar leaves ~20 bits of slack.
* the host's cell_power_table (long double, 64-bit significand): B's sixths, the 32
  products and 15 sums, and the divisions, each 2^-64 of at most S: below 2^-58 S,
  plus the rounding to double.  So |host - exact| and |got - host| are both held to
  1 ulp(exact) + 2^-58 S.

Host build of tests/native/cell_table_host.hip; the GPU test
(tests/test_gpu_plasma_update.py) holds the kernel's table array_equal to this
host run, which is what makes these CPU bars the kernel's."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = C.POINTER(C.c_double)
NF, REC = 8, 96
M6 = ((1, 4, 1, 0), (-3, 0, 3, 0), (3, -6, 3, 0), (-1, 3, -3, 1))


def load_harness():
    """libcell_table_host.so, compiled from tests/native/cell_table_host.hip (host code only)."""
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", "libcell_table_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "cell_table_host.hip")])
    L = C.CDLL(out)
    for f in (L.ct_record_table, L.ct_host_table):
        f.argtypes = [_dp, C.c_int, C.c_int, C.c_double, C.c_double, _dp]
        f.restype = None
    assert L.ct_nf() == NF and L.ct_rec() == REC
    return L


def run_table(fn, coef, nR, nZ, hR, hZ):
    """coef: (nZ + 2, nR + 2, NF) interleaved node coefficients -> (nZ - 1, nR - 1, 6, 4, 4)"""
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    assert coef.shape == (nZ + 2, nR + 2, NF)
    out = np.full((nZ - 1, nR - 1, 6, 4, 4), np.nan)
    fn(coef.ctypes.data_as(_dp), nR, nZ, float(hR), float(hZ), out.ctypes.data_as(_dp))
    return out


@pytest.fixture(scope="module")
def H():
    return load_harness()


def _ilog2(x: Fraction) -> int:
    """floor(log2 x), x > 0, exactly"""
    n, d = x.numerator, x.denominator
    e = n.bit_length() - d.bit_length()
    ge = n >= (d << e) if e >= 0 else (n << -e) >= d
    return e if ge else e - 1


def ulp(x: Fraction) -> Fraction:
    """the spacing of doubles at |x| (normal range); 0 at 0"""
    if x == 0:
        return Fraction(0)
    return Fraction(2) ** (_ilog2(abs(x)) - 52)


def exact_table(coef, nR, nZ, hR, hZ):
    """(exact, S) per entry, as object arrays of Fraction, shape (nZ - 1, nR - 1, 6, 4, 4).
    The integer-weighted sums run on the coefficients scaled to integers by one power of
    two (exact: doubles are dyadic), the quotient is a Fraction."""
    fr = [[[Fraction(float(coef[z, r, f])) for f in range(6)] for r in range(nR + 2)] for z in range(nZ + 2)]
    K = max(q.denominator.bit_length() - 1 for pl in fr for row in pl for q in row)
    ci = [[[int(q * (1 << K)) for q in row] for row in pl] for pl in fr]
    FR, FZ = Fraction(float(hR)), Fraction(float(hZ))
    den = [[Fraction(36 << K) * FR ** i * FZ ** j for i in range(4)] for j in range(4)]
    W = [[[(M6[j][b] * M6[i][a], b, a) for b in range(4) for a in range(4) if M6[j][b] * M6[i][a]]
          for i in range(4)] for j in range(4)]
    ex = np.empty((nZ - 1, nR - 1, 6, 4, 4), dtype=object)
    S = np.empty_like(ex)
    for z in range(nZ - 1):
        for r in range(nR - 1):
            for f in range(6):
                c = [[ci[z + b][r + a][f] for a in range(4)] for b in range(4)]
                for j in range(4):
                    for i in range(4):
                        n = s = 0
                        for m, b, a in W[j][i]:
                            t = m * c[b][a]
                            n += t
                            s += abs(t)
                        ex[z, r, f, j, i] = n / den[j][i]
                        S[z, r, f, j, i] = s / den[j][i]
    return ex, S


def make_coefs(nR, nZ, seed):
    """mixed signs and magnitudes 1e-8 .. 1e3; a field of size ~40 with ulp-scale noise
    (the ln ne case); exact zeros, whole and sprinkled; smooth fields"""
    rng = np.random.default_rng(seed)
    shp = (nZ + 2, nR + 2)
    zz, rr = np.meshgrid(np.linspace(-1, 1, shp[0]), np.linspace(0.5, 1.5, shp[1]), indexing="ij")
    c = np.zeros(shp + (NF,))
    c[..., 0] = rng.choice([-1.0, 1.0], shp) * 10.0 ** rng.uniform(-8, 3, shp)
    c[..., 1] = 40.0 * (1.0 + rng.integers(-4, 5, shp) * 2.0 ** -52)
    c[..., 2] = 0.0
    c[..., 3] = 44.0 - 6.0 * (rr - 1.0) ** 2 - 5.0 * zz ** 2 + 1e-13 * rng.standard_normal(shp)
    c[..., 4] = np.where(rng.random(shp) < 0.3, 0.0, rng.standard_normal(shp) * 10.0 ** rng.uniform(-8, 3, shp))
    c[..., 5] = ((rr - 1.0) ** 2 + zz ** 2) / 0.36
    return c


GRIDS = ((2, 2, 0.8, 0.3), (6, 5, 0.0321, 0.0417), (17, 29, 1.6 / 16, 1.7 / 28))


@pytest.mark.parametrize("nR,nZ,hR,hZ", GRIDS, ids=lambda v: str(v))
def test_record_function_against_exact(H, nR, nZ, hR, hZ):
    assert hR != hZ
    coef = make_coefs(nR, nZ, 100 * nR + nZ)
    got = run_table(H.ct_record_table, coef, nR, nZ, hR, hZ)
    host = run_table(H.ct_host_table, coef, nR, nZ, hR, hZ)
    assert np.isfinite(got).all() and np.isfinite(host).all()
    ex, S = exact_table(coef, nR, nZ, hR, hZ)
    t80, t58 = Fraction(1, 1 << 80), Fraction(1, 1 << 58)
    worst = dict(dd_ulp=0.0, dd_S=0.0, host_ulp=0.0, host_S=0.0)
    bad = []
    for idx in np.ndindex(ex.shape):
        e, s, u = ex[idx], S[idx], ulp(ex[idx])
        dg = abs(Fraction(float(got[idx])) - e)
        dh = abs(Fraction(float(host[idx])) - e)
        dgh = abs(Fraction(float(got[idx])) - Fraction(float(host[idx])))
        if s == 0:  # an all-zero stencil: exactly zero from both
            assert got[idx] == 0.0 and host[idx] == 0.0, idx
            continue
        if u:
            worst["dd_ulp"] = max(worst["dd_ulp"], float(dg / u))
            worst["host_ulp"] = max(worst["host_ulp"], float(dh / u))
        worst["dd_S"] = max(worst["dd_S"], float(max(dg - u, 0) / s))
        worst["host_S"] = max(worst["host_S"], float(max(dh - u, 0) / s))
        if not (dg <= u + t80 * s and dh <= u + t58 * s and dgh <= u + t58 * s):
            bad.append((idx, float(dg), float(dh), float(dgh), float(u), float(s)))
    print(f"grid {nR}x{nZ}: cell_record max |err| {worst['dd_ulp']:.3f} ulp(exact), beyond 1 ulp "
          f"{worst['dd_S']:.3e} S (bar 2^-80 = {2.0 ** -80:.3e}); cell_power_table max |err| "
          f"{worst['host_ulp']:.3f} ulp(exact), beyond 1 ulp {worst['host_S']:.3e} S "
          f"(bar 2^-58 = {2.0 ** -58:.3e})")
    assert not bad, bad[:5]

