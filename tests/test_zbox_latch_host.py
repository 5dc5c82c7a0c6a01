"""The trajectory kernel's dead-box latch (torj_k_traj.hpp traj_run) on CPU, in
both forms of the node exponent (TORJ_NODE_GAMMA_LIN 1, the default, and 0):

* zero_box_flag is monotone along a sequence of points: once a prefix's flag
  is false, the flag of every longer prefix, the whole sequence included, is
  false;
* traj_run's latched bookkeeping (stop adding to the boxes of a wave once no
  lane still in the loop has a true flag, kill those boxes) writes the flags the
  unlatched bookkeeping writes, at several cadences and wave widths, with lanes
  that leave the loop early.

Over 200 000 random sequences per form: random walks of stage points, sequences
whose points sit within 1e-9 (relative) of each threshold of zero_box_flag, and
sequences with NaN / infinite inputs.  Host build of
tests/native/zbox_latch_host.hip (the device takes v_max_f64 / v_min_f64 where
the host takes fmax / fmin; non-finite inputs are the box's chk word's business
in both)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_skip_proofs_host import _threshold_points

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
FIELDS = ("lnTe", "Y", "Npar", "N2")
N_SEQ = 200000
STRIDE = 4  # stage points per step
# (points per sequence, sequences): 2-step, 6-step and whole 60-step blocks
K_SHARE = ((8, 100000), (24, 90000), (240, 10000))
# the trips after which a wave looks at its flags: the kernel's (1, 16), every
# trip, single looks early and late, and none (the unlatched bookkeeping itself)
CADENCES = ((1, 16), tuple(range(1, 61)), (1,), (2, 5), (16,), (59, 60), ())


def _p(a):
    return a.ctypes.data_as(_dp)


def _pi(a):
    return a.ctypes.data_as(_ip)


@pytest.fixture(scope="module", params=[1, 0], ids=["gamma_lin1", "gamma_lin0"])
def H(request):
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", f"libzbox_latch_host{request.param}.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # libwarm_host.so's flags (tests/native/Makefile), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           f"-DTORJ_NODE_GAMMA_LIN={request.param}",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "zbox_latch_host.hip")])
    L = C.CDLL(out)
    L.zl_prefix.argtypes = [C.c_int, C.c_int] + [_dp] * 4 + [_ip] * 3
    L.zl_latched.argtypes = [C.c_int] * 5 + [_ip, _ip] + [_dp] * 4 + [_ip, _ip]
    assert L.zl_gamma_lin() == request.param
    return L


def _random_walks(nb, k, rng):
    """nb sequences of k points: a random centre (the ranges of
    test_skip_proofs_host._boxes) and a drift plus jitter per input, relative
    sizes log-uniform 1e-12 - 0.3 per sequence and input, so that sequences
    cross the flag's thresholds at every scale"""
    c = dict(Te=np.exp(rng.uniform(0.0, np.log(3e4), nb)), Y=rng.uniform(0.05, 1.5, nb),
             Npar=rng.uniform(-0.99, 0.99, nb), Np2=np.exp(rng.uniform(np.log(1e-6), np.log(1.2), nb)))
    v = {}
    for f in c:
        drift = np.exp(rng.uniform(np.log(1e-12), np.log(0.3), nb)) * rng.choice([-1.0, 1.0], nb)
        jit = np.exp(rng.uniform(np.log(1e-12), np.log(0.3), nb))
        t = np.linspace(0.0, 1.0, k)[None, :]
        v[f] = c[f][:, None] * (1.0 + drift[:, None] * t + jit[:, None] * rng.uniform(-1.0, 1.0, (nb, k)))
    with np.errstate(all="ignore"):
        return dict(lnTe=np.log(v["Te"]), Y=v["Y"], Npar=v["Npar"], N2=v["Npar"] ** 2 + v["Np2"])


def _threshold_walks(nb, k, rng):
    """nb sequences of k points all within 1e-9 (relative, per input; widths
    log-uniform from 1e-16) of a point on one of zero_box_flag's thresholds
    (test_skip_proofs_host._threshold_points: Te = 20 eV, m Y = sqrt(1 - N_par^2),
    m Y = (1 + 760 / mu)(1 + |N_par|), N_par^2 = 1 and the flag's bounds below it,
    N_perp^2 = 0, ln Te = 300 and 700)"""
    rows = np.vstack(list(_threshold_points().values()))
    base = rows[rng.integers(0, len(rows), nb)]
    P = {}
    for j, f in enumerate(FIELDS):
        wd = np.exp(rng.uniform(np.log(1e-16), np.log(1e-9), nb))
        P[f] = base[:, j][:, None] * (1.0 + wd[:, None] * rng.uniform(-1.0, 1.0, (nb, k)))
    return P


def _with_non_finite(P, rng, share=0.5):
    """a NaN, +inf or -inf in one input at one position, in `share` of the sequences"""
    nb, k = P["lnTe"].shape
    rows = np.flatnonzero(rng.uniform(size=nb) < share)
    for b in rows:
        P[FIELDS[rng.integers(0, 4)]][b, rng.integers(0, k)] = (np.nan, np.inf, -np.inf)[rng.integers(0, 3)]
    return P


def _sequences(k, nb, rng):
    """nb sequences of k points: 60 % random walks, 30 % threshold walks, 10 %
    of either with a non-finite input"""
    n_t = (3 * nb) // 10
    n_nf = nb // 10
    n_r = nb - n_t - n_nf
    parts = [_random_walks(n_r, k, rng), _threshold_walks(n_t, k, rng),
             _with_non_finite(_random_walks(n_nf - n_nf // 2, k, rng), rng, 1.0),
             _with_non_finite(_threshold_walks(n_nf // 2, k, rng), rng, 1.0)]
    return {f: np.ascontiguousarray(np.vstack([p[f] for p in parts]), dtype=float) for f in FIELDS}


def _prefix(H, P):
    nb, k = P["lnTe"].shape
    fin, ff, back = (np.zeros(nb, dtype=np.int32) for _ in range(3))
    H.zl_prefix(nb, k, *[_p(P[f]) for f in FIELDS], _pi(fin), _pi(ff), _pi(back))
    return fin == 1, ff, back


def _latched(H, P, cad, wave, length):
    nb, k = P["lnTe"].shape
    flag, lat = np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int32)
    cad = np.ascontiguousarray(cad, dtype=np.int32)
    H.zl_latched(nb, k, STRIDE, wave, len(cad), _pi(cad), _pi(np.ascontiguousarray(length, dtype=np.int32)),
                 *[_p(P[f]) for f in FIELDS], _pi(flag), _pi(lat))
    return flag == 1, lat


@pytest.fixture(scope="module")
def seqs():
    """the sequences of both tests (the same for both forms of the node exponent): made once"""
    rng = np.random.default_rng(2611)
    assert sum(nb for _, nb in K_SHARE) == N_SEQ
    return [_sequences(k, nb, rng) for k, nb in K_SHARE]


def test_false_flag_stays_false(H, seqs):
    """No sequence has a prefix with a false flag before a longer prefix (the
    whole sequence included) with a true one; and the sweep is live: flags go
    false in the middle of at least 5 000 sequences, at least 20 000 stay true
    and at least 20 000 are false from the first point."""
    n_mid = n_true = n_first = 0
    for P in seqs:
        fin, ff, back = _prefix(H, P)
        bad = np.flatnonzero(back > 0)
        assert bad.size == 0, (f"flag false after {ff[bad[0]]} points, true again after {back[bad[0]]}",
                               {f: P[f][bad[0]][:back[bad[0]]] for f in FIELDS})
        assert not (fin & (ff > 0)).any()
        n_mid += int((ff > 1).sum())
        n_true += int(fin.sum())
        n_first += int((ff == 1).sum())
        print(f"k {P['lnTe'].shape[1]}: {len(fin)} sequences, true to the end {fin.mean():.3f}, "
              f"false from the first point {(ff == 1).mean():.3f}, going false later {(ff > 1).mean():.3f}")
    assert n_mid >= 5000 and n_true >= 20000 and n_first >= 20000, (n_mid, n_true, n_first)


def test_latched_flags_equal_unlatched(H, seqs):
    """traj_run's latched bookkeeping writes the unlatched flags: waves of 1, 4
    and 64 lanes, every cadence of CADENCES, all lanes running the whole block
    and lanes leaving the loop at random trips; the unlatched reference is the
    flag of the points each lane added (zl_prefix over its own trips).  The
    latch is seen to fire."""
    rng = np.random.default_rng(77)
    fired = 0
    for P in seqs:
        nb, k = P["lnTe"].shape
        trips = k // STRIDE
        full = np.full(nb, trips, dtype=np.int32)
        ragged = rng.integers(1, trips + 1, nb).astype(np.int32)
        for length in (full, ragged):
            # the unlatched flag: the box of the points of the lane's own trips
            # (a lane's points past its last trip are never added: hold them at
            # its last point)
            Q = {f: P[f].copy() for f in FIELDS}
            idx = np.minimum(np.arange(k)[None, :], (length * STRIDE - 1)[:, None])
            Q = {f: np.ascontiguousarray(np.take_along_axis(Q[f], idx, 1)) for f in FIELDS}
            ref, _, _ = _prefix(H, Q)
            for wave in (1, 4, 64):
                for cad in CADENCES:
                    got, lat = _latched(H, P, [c for c in cad if c <= trips], wave, length)
                    assert np.array_equal(got, ref), (wave, cad, np.flatnonzero(got != ref)[:5])
                    assert not (got & (lat > 0)).any()
                    if cad:
                        fired += int((lat > 0).sum())
                    else:
                        assert not lat.any()
    print(f"{fired} boxes latched over all cadences")
    assert fired > 100000
