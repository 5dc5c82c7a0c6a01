"""Ray profiles (torj_ray_profile[_device], T.ray_profile) on the GPU: one row of 25
columns per saved point of every ray -- against the existing multi-beam trace with the
same lanes per ray (bit for bit), the NaN pattern, N along the ray and every derived
column against the CPU oracle, through two plasmas, the device form back to back, no
absorption, and the documented torj_alpha_warm recipe.

Workload (tests/test_ray_profile_capi.py, which pins its preconditions with the oracle):
the synthetic tokamak and SETUP's launch point, 32 rays of five beams taken from the
default 46-ray fan -- 13 + 5 + 0 + 1 + 13, so beams end inside a wave at both 4 and 64
rays per wave and one is empty -- 12 000 steps of 1e-4 m with checks every 120 and a row
every 1 000 steps: 13 rows.  Rays end OK, LEFT_PLASMA (11 640, 11 760 steps) and
ABSORBED (5 880 steps).  The two profiles and the oracle's traces are computed once."""
import numpy as np
import pytest

from test_gpu_parity import TAU_FLOOR, _compare_trace
from test_ray_profile_capi import BEAMS, CHUNK, DS, N_ROWS, N_STEPS, OFF, STRIDE, oracle_beams, workload

pytestmark = pytest.mark.gpu

KW = dict(ds=DS, n_steps=N_STEPS, chunk_steps=CHUNK, traj_stride=STRIDE)
NB = len(BEAMS)
C = {name: c for c, name in enumerate(("x", "y", "z", "Nx", "Ny", "Nz", "tau", "s", "P", "alpha", "dP_ds", "psi",
                                       "ne", "Te", "Bx", "By", "Bz", "B_abs", "X", "Y", "N_par", "N_abs", "Ns2",
                                       "Lambda", "dLambda_dN"))}


def beam_of(i):
    return next(k for k in range(NB) if OFF[k] <= i < OFF[k + 1])


@pytest.fixture(scope="module")
def b(T, hplasma):
    return workload(T, hplasma)


def profile(T, p, b, sched, **kw):
    try:
        p.set_sched(sched)
        return T.ray_profile(p, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], **{**KW, "s0": b["s0"], **kw})
    finally:
        p.set_sched(-1)


@pytest.fixture(scope="module")
def prof16(gpu, T, hplasma, b):
    """the profile with 16 lanes per ray (torj_set_sched 2)"""
    return profile(T, hplasma, b, 2)


@pytest.fixture(scope="module")
def prof1(gpu, T, hplasma, b):
    """... with one lane per ray (torj_set_sched 0)"""
    return profile(T, hplasma, b, 0)


@pytest.fixture(scope="module")
def oracle_full(oplasma, b):
    """the oracle's traces of the beams over all 12 000 steps; the X-mode beam's with make_ray's samples"""
    res = oracle_beams(oplasma, b)
    res[0] = oplasma.trace(b["xp"][:13], b["Np"][:13], b["omega"][0], b["mode"][0], DS, N_STEPS, chunk_steps=CHUNK,
                           samples=True)
    return res


def test_shape_and_columns(T, prof16):
    r = prof16
    assert r.table.shape == (32, N_ROWS, 25) and N_ROWS == 13
    assert r.columns == tuple(C) == T.PROFILE_COLUMNS
    assert r.state.shape == (32, 7) and r.status.shape == (32,) and r.steps.shape == (32,)
    assert np.array_equal(r["N_par"], r.table[:, :, 20], equal_nan=True)


@pytest.mark.parametrize("lanes", [16, 1])
def test_equals_trace_beams_same_lanes(T, hplasma, b, prof16, prof1, lanes):
    """Check 1: the trace kernel is k_trace_beams' code, so state, status, steps and the columns
    x, y, z, tau, s of rows 1.. are the bits torj_trace_beams gives with the same lanes per ray;
    row 0 is (x0, N0, 0, s0)."""
    r = prof16 if lanes == 16 else prof1
    try:
        hplasma.set_sched(2 if lanes == 16 else 0)
        m = T.trace_beams(hplasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], s0=b["s0"], **KW)
    finally:
        hplasma.set_sched(-1)
    assert np.array_equal(r.state, m.state)
    assert np.array_equal(r.status, m.status)
    assert np.array_equal(r.steps, m.steps)
    assert m.traj.shape == (32, N_ROWS - 1, 5)
    for c, name in enumerate(("x", "y", "z", "tau", "s")):
        same = np.array_equal(r[name][:, 1:], m.traj[:, :, c], equal_nan=True)
        if not same:
            print(f"lanes {lanes}: column {name} differs from traj by "
                  f"{np.nanmax(np.abs(r[name][:, 1:] - m.traj[:, :, c])):.3e}")
        assert same
    assert np.array_equal(r.table[:, 0, 0:3], b["xp"])
    assert np.array_equal(r.table[:, 0, 3:6], b["Np"])
    assert (r["tau"][:, 0] == 0.0).all()
    assert np.array_equal(r["s"][:, 0], b["s0"])
    # the last stored row of a ray that stopped on a row is its final state
    on_row = np.flatnonzero(r.steps % STRIDE == 0)
    assert len(on_row)
    for i in on_row:
        assert np.array_equal(r.table[i, r.steps[i] // STRIDE, 0:7], r.state[i])


@pytest.mark.parametrize("lanes", [16, 1])
def test_nan_pattern(T, prof16, prof1, oracle_full, lanes):
    """Check 2: row k of ray i is finite in all 25 columns iff k * 1000 <= steps[i], all NaN otherwise."""
    r = prof16 if lanes == 16 else prof1
    steps_o = np.concatenate([oracle_full[k]["steps"] for k in sorted(oracle_full)])
    assert np.array_equal(r.steps, steps_o)
    assert (r.steps % STRIDE != 0).any() and (r.steps == N_STEPS).any()
    for i in range(32):
        for k in range(N_ROWS):
            row = r.table[i, k]
            if k * STRIDE <= r.steps[i]:
                assert np.isfinite(row).all(), (i, k, row)
            else:
                assert np.isnan(row).all(), (i, k, row)
    assert {T.OK, T.LEFT_PLASMA, T.ABSORBED} <= set(r.status.tolist())


def test_empty_beam_changes_nothing(T, hplasma, b, prof16):
    """... and the same rays without the empty beam give the same table"""
    keep = [k for k in range(NB) if OFF[k] < OFF[k + 1]]
    off = np.concatenate([[0], np.cumsum([OFF[k + 1] - OFF[k] for k in keep])])
    b2 = dict(b, off=off, omega=[b["omega"][k] for k in keep], mode=[b["mode"][k] for k in keep])
    r = profile(T, hplasma, b2, 2)
    assert np.array_equal(r.table, prof16.table, equal_nan=True)
    assert np.array_equal(r.steps, prof16.steps)


class _Rows:
    """row k of the rays `sel` as _compare_trace reads a trace's final state"""

    def __init__(self, r, sel, k, o):
        self.state = r.table[sel, k, 0:7]
        self.status, self.steps = o["status"], o["steps"]


@pytest.mark.parametrize("k", [1, 4, 9, 12])
def test_N_along_the_ray_matches_oracle(T, oplasma, b, prof16, prof1, oracle_full, k):
    """Check 3: a prefix run of RK4 is the same run, so the oracle's final (x, N, tau) after 1000 k
    steps is row k, at _compare_trace's bars, for the rays that reach step 1000 k (the oracle's steps)."""
    res = oracle_full if k * STRIDE == N_STEPS else oracle_beams(oplasma, b, n_steps=k * STRIDE)
    n_checked = 0
    for r in (prof16, prof1):
        for kb, o in res.items():
            reach = np.flatnonzero(o["steps"] == k * STRIDE)
            sel = OFF[kb] + reach
            gone = OFF[kb] + np.flatnonzero(o["steps"] != k * STRIDE)
            assert np.isnan(r.table[gone, k]).all()
            if not len(sel):
                continue
            o_sel = dict(state=o["state"][reach], status=o["status"][reach], steps=o["steps"][reach])
            _compare_trace(_Rows(r, sel, k, o_sel), o_sel)
            n_checked += len(sel)
    assert n_checked >= 2 * (13 if k == 12 else 31)


def test_derived_columns_match_oracle(T, O, hplasma, oplasma, b, prof16):
    """Check 4: columns 8-24 against the oracle's functions at the GPU's own (x, N) of every finite
    row, at the bars of test_fields_match_oracle (points inside the box),
    test_dispersion_and_gradients_match_oracle and test_albajar_matches_oracle_along_rays;
    column 22 against O.refractive_index_sq at the table's own X, Y, N_par (1e-13); P, dP/ds and
    |N| are exact functions of other columns of their row (<= 2 ulp)."""
    r = prof16
    c_ne = np.abs(hplasma.coefs("lnne")).max()
    c_te = np.abs(hplasma.coefs("lnTe")).max()
    worst = dict(B=0.0, ne=0.0, Te=0.0, psi=0.0, X=0.0, Y=0.0, Npar=0.0, Ns2=0.0, D=0.0, gn=0.0, alpha=0.0)
    n_rows = 0
    for i in range(32):
        kb = beam_of(i)
        om, mode = b["omega"][kb], b["mode"][kb]
        for k in range(r.steps[i] // STRIDE + 1):
            t = r.table[i, k]
            x, N = t[0:3], t[3:6]
            n_rows += 1
            R = np.hypot(x[0], x[1])
            assert hplasma.R_coords[0] <= R <= hplasma.R_coords[-1]
            assert hplasma.Z_coords[0] <= x[2] <= hplasma.Z_coords[-1]
            B = oplasma.B_spline(x)
            e = np.abs(t[14:17] - B).max() / np.linalg.norm(B)
            worst["B"] = max(worst["B"], e)
            assert e <= 1e-13
            assert abs(t[17] - np.linalg.norm(B)) <= 1e-13 * np.linalg.norm(B)
            ne, Te = oplasma.n_e(x), oplasma.T_e(x)
            worst["ne"] = max(worst["ne"], abs(t[12] - ne) / ne)
            worst["Te"] = max(worst["Te"], abs(t[13] - Te) / Te)
            assert abs(t[12] - ne) < 1e-13 * c_ne * ne
            assert abs(t[13] - Te) < 1e-13 * c_te * Te
            psi = oplasma.evaluate("psi", x)
            worst["psi"] = max(worst["psi"], abs(t[11] - psi))
            assert abs(t[11] - psi) < 1e-13 * max(1, abs(t[11]))
            X, Y, Npar, _ = oplasma.eval_plasma(x, N, om)
            worst["X"] = max(worst["X"], abs(t[18] - X) / X)
            worst["Y"] = max(worst["Y"], abs(t[19] - Y) / Y)
            worst["Npar"] = max(worst["Npar"], abs(t[20] - Npar))
            assert abs(t[18] - X) < 1e-13 * c_ne * X
            assert abs(t[19] - Y) < 1e-13 * Y
            assert abs(t[20] - Npar) < 1e-13
            ns2 = O.refractive_index_sq(t[18], t[19], t[20], mode)
            worst["Ns2"] = max(worst["Ns2"], abs(t[22] - ns2))
            assert abs(t[22] - ns2) <= 1e-13 * max(1.0, abs(ns2))
            D = oplasma.dispersion_relation(x, N, om, mode)
            worst["D"] = max(worst["D"], abs(t[23] - D))
            assert abs(t[23] - D) <= 1e-12 * max(1.0, abs(D))
            gn = oplasma.grad_norm(x, N, om, mode)
            worst["gn"] = max(worst["gn"], abs(t[24] - gn))
            assert abs(t[24] - gn) <= 1e-10 * max(1.0, gn)
            ao = oplasma.alpha_approx(x, N, om, mode)
            if ao != 0:
                worst["alpha"] = max(worst["alpha"], abs(t[9] - ao) / abs(ao))
            assert abs(t[9] - ao) <= 1e-10 * abs(ao) + 1e-30
            # exact functions of the row's own columns
            for got, want in ((t[8], np.exp(-t[6])), (t[10], t[8] * t[9]), (t[21], np.sqrt(N @ N))):
                assert abs(got - want) <= 2 * np.spacing(abs(want)), (i, k, got, want)
            # the cold index the ray sits on: Lambda = |N|^2 - Ns2
            assert abs(t[23] - (t[21] ** 2 - t[22])) <= 1e-12
    print(f"{n_rows} rows; worst: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert n_rows == int((prof16.steps // STRIDE + 1).sum())
    assert np.nanmax(r["alpha"][:13]) > 0.0  # the X-mode beam is absorbed


def test_dP_ds_is_make_rays(T, oplasma, b, prof16, prof1, oracle_full):
    """Check 5: column 10 of the X-mode beam against make_ray's dP/ds samples at steps 1000 k
    (1e-10 relative; below TAU_FLOOR per metre absolutely: over the ray's 1.2 m such a dP/ds moves P
    by less than tau's own floor).  Row 0 carries P alpha at the entry point; the reference's
    leading 0 there is make_ray's padding, not alpha, and is not imitated."""
    o = oracle_full[0]
    smp = o["samples"]
    assert (smp[:, 0, 1] == 0.0).all()  # the oracle imitates the padding
    for r in (prof16, prof1):
        n_checked = 0
        for i in range(13):
            for k in range(1, r.steps[i] // STRIDE + 1):
                want = smp[i, k * STRIDE, 1]
                got = r["dP_ds"][i, k]
                assert abs(got - want) <= 1e-10 * max(abs(want), TAU_FLOOR), (i, k, got, want)
                n_checked += 1
            a0 = oplasma.alpha_approx(b["xp"][i], b["Np"][i], b["omega"][0], 1)
            assert abs(r["dP_ds"][i, 0] - a0) <= 1e-10 * abs(a0) + 1e-30
            assert r["P"][i, 0] == 1.0
        assert n_checked == 13 * 11
        assert np.nanmax(r["dP_ds"][:13, 1:]) > 0.0


def test_through_two_plasmas(T, hplasma, b, prof16):
    """Check 6: the beams through plasmas = [a, b], alternating: each beam's rows are the bits of
    a one-plasma call on its own plasma (16 lanes per ray in all three calls)."""
    from torj_hip import synthetic as S

    pb = T.Plasma(*S.plasma_args(S.circular_tokamak(Te0=6000, ne_scale=0.6)))
    bp = [k % 2 for k in range(NB)]
    try:
        hplasma.set_sched(2), pb.set_sched(2)
        m = T.ray_profile(hplasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], s0=b["s0"],
                          plasmas=[hplasma, pb], beam_plasma=bp, **KW)
        own_b = T.ray_profile(pb, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], s0=b["s0"], **KW)
    finally:
        hplasma.set_sched(-1)
    differs = False
    for k in range(NB):
        sl = slice(OFF[k], OFF[k + 1])
        own = own_b if bp[k] else prof16
        assert np.array_equal(m.table[sl], own.table[sl], equal_nan=True)
        assert np.array_equal(m.state[sl], own.state[sl])
        assert np.array_equal(m.status[sl], own.status[sl]) and np.array_equal(m.steps[sl], own.steps[sl])
        if bp[k] and sl.start < sl.stop:
            differs |= not np.array_equal(m["Te"][sl], prof16["Te"][sl], equal_nan=True)
    assert differs  # (the second plasma is another plasma)


def test_device_form_back_to_back(T, hplasma, b, prof16):
    """Check 7: two torj_ray_profile_device calls on one stream with no sync between them, the host
    tables overwritten with the second call's values as soon as the first has returned: each call
    saw its own tables -- its outputs are those of the same call enqueued and checked alone -- and
    they are the host form's rows of its rays (16 lanes per ray everywhere)."""
    import torch

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    L = T.lib()
    cfg = T._lib.TraceCfg(0.0, 0, DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, STRIDE)
    sets = ((0, 3), (3, 5))  # beams 0..2 (18 rays), beams 3..4 (14 rays)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=torch.float64)

    class Call:
        def __init__(self, lo, hi):
            self.sl = slice(OFF[lo], OFF[hi])
            self.n, self.nb = OFF[hi] - OFF[lo], hi - lo
            self.x0, self.N0, self.s0 = t(b["xp"][self.sl].T), t(b["Np"][self.sl].T), t(b["s0"][self.sl])
            self.prof = torch.zeros((N_ROWS, 25, self.n), dtype=torch.float64, device=dev)
            self.state = torch.empty((7, self.n), dtype=torch.float64, device=dev)
            self.status = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.steps = torch.empty(self.n, dtype=torch.int32, device=dev)

        def enqueue(self, off, om, md):
            T._lib.check(L.torj_ray_profile_device(
                hplasma.handle, 0, None, None, cfg, self.nb, T._lib.iptr(off), T._lib.dptr(om), T._lib.iptr(md),
                self.x0.data_ptr(), self.N0.data_ptr(), self.s0.data_ptr(), N_ROWS, self.prof.data_ptr(),
                self.state.data_ptr(), self.status.data_ptr(), self.steps.data_ptr(), stream.cuda_stream))

        def out(self):
            return [a.cpu().numpy() for a in (self.prof, self.state, self.status, self.steps)]

    def tables(lo, hi):
        return (np.array(OFF[lo:hi + 1], dtype=np.int32) - OFF[lo], np.array(b["omega"][lo:hi]),
                np.array(b["mode"][lo:hi], dtype=np.int32))

    off, om, md = np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(8, dtype=np.int32)
    calls, want = [], []
    try:
        hplasma.set_sched(2)
        # separately synchronised calls, each with tables of its own
        for lo, hi in sets:
            c = Call(lo, hi)
            c.enqueue(*tables(lo, hi))
            assert L.torj_trace_check(hplasma.handle, stream.cuda_stream) == 0
            want.append(c.out())
        # back to back: one set of table arrays, overwritten between the calls
        for lo, hi in sets:
            off[:], om[:], md[:] = 0, 0.0, 0
            off[:hi - lo + 1] = np.array(OFF[lo:hi + 1]) - OFF[lo]
            om[:hi - lo], md[:hi - lo] = b["omega"][lo:hi], b["mode"][lo:hi]
            calls.append(Call(lo, hi))
            calls[-1].enqueue(off, om, md)
        assert L.torj_trace_check(hplasma.handle, stream.cuda_stream) == 0
        # state, status and steps are optional: NULL leaves the table as it is
        c3 = Call(3, 5)
        o3, m3 = np.array([0, 1, 14], dtype=np.int32), np.array(b["mode"][3:5], dtype=np.int32)
        T._lib.check(L.torj_ray_profile_device(
            hplasma.handle, 0, None, None, cfg, 2, T._lib.iptr(o3), T._lib.dptr(np.array(b["omega"][3:5])),
            T._lib.iptr(m3), c3.x0.data_ptr(), c3.N0.data_ptr(), c3.s0.data_ptr(), N_ROWS, c3.prof.data_ptr(),
            None, None, None, stream.cuda_stream))
        assert L.torj_trace_check(hplasma.handle, stream.cuda_stream) == 0
    finally:
        hplasma.set_sched(-1)
    for c, ref in zip(calls, want):
        for a, r in zip(c.out(), ref):
            assert np.array_equal(a, r, equal_nan=True)
        # against the host form's rows of the same rays: the trace's outputs and every column but
        # alpha and P alpha are the same bits (a ray's results do not depend on the launch's other
        # beams); abs_albajar_fast's per-wave choices see the rays that share its wave in the point
        # kernel, so those two columns agree to the alpha bar between launches of differing rays
        table = c.out()[0].transpose(2, 0, 1)
        host = prof16.table[c.sl]
        print("columns whose bits differ from the host form's:",
              [k for k in range(25) if not np.array_equal(table[:, :, k], host[:, :, k], equal_nan=True)])
        rest = [k for k in range(25) if k not in (C["alpha"], C["dP_ds"])]
        assert np.array_equal(table[:, :, rest], host[:, :, rest], equal_nan=True)
        for k in (C["alpha"], C["dP_ds"]):
            fin = np.isfinite(host[:, :, k])
            assert np.array_equal(fin, np.isfinite(table[:, :, k]))
            assert (np.abs(table[:, :, k][fin] - host[:, :, k][fin]) <= 1e-10 * np.abs(host[:, :, k][fin]) + 1e-30).all()
        assert np.array_equal(c.out()[1].T, prof16.state[c.sl])
        assert np.array_equal(c.out()[2], prof16.status[c.sl]) and np.array_equal(c.out()[3], prof16.steps[c.sl])
    assert np.array_equal(c3.prof.cpu().numpy(), want[1][0], equal_nan=True)


def test_absorption_0(gpu, T, hplasma, b):
    """Check 8: without absorption tau, alpha and dP/ds are zero and P is 1 on the stored rows, and
    x, N are the absorption = 0 trace's."""
    r = profile(T, hplasma, b, 0, absorption=False, s0=None)
    try:
        hplasma.set_sched(0)
        m = T.trace_beams(hplasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], absorption=False, **KW)
    finally:
        hplasma.set_sched(-1)
    assert np.array_equal(r.state, m.state) and np.array_equal(r.steps, m.steps)
    assert np.array_equal(r.status, m.status) and T.ABSORBED not in set(r.status.tolist())
    assert np.array_equal(r.table[:, 1:, 0:3], m.traj[:, :, 0:3], equal_nan=True)
    fin = np.isfinite(r["x"])
    assert np.array_equal(fin, np.arange(N_ROWS)[None, :] * STRIDE <= r.steps[:, None])
    for name in ("tau", "alpha", "dP_ds"):
        assert (r[name][fin] == 0.0).all()
    assert (r["P"][fin] == 1.0).all()
    assert np.isfinite(r.table[fin]).all() and np.isnan(r.table[~fin]).all()
    # s0 = None: s counts from the entry point
    assert np.array_equal(r["s"][:, 1:], m.traj[:, :, 4], equal_nan=True)
    assert (r["s"][:, 0] == 0.0).all()
    # N along the ray: the last stored row of a ray that stopped on a row
    for i in np.flatnonzero(r.steps % STRIDE == 0):
        assert np.array_equal(r.table[i, r.steps[i] // STRIDE, 3:6], m.state[i, 3:6])


def test_alpha_warm_recipe(T, oplasma, b, prof16):
    """Check 9: the documented use -- columns X, Y, |N|, N_par, T_e and 1 / |dLambda/dN| of an O-mode
    ray's stored rows into torj_alpha_warm (iwarm 1) -- against the oracle's weakly relativistic alpha
    at the row's (x, N), at test_gpu_warm's point bar for iwarm 1: 1e-7 relative to |alpha| plus the
    rounding floor of Im(N_perp^2), on its domain (T_e >= 1 keV, warmdisp converged)."""
    import warnings

    import warm_ref as W

    i, kb = OFF[4] + 2, 4
    om, mode = b["omega"][kb], b["mode"][kb]
    assert mode == -1 and prof16.steps[i] == N_STEPS
    t = prof16.table[i]
    a, n2 = T.alpha_warm(np.full(N_ROWS, om), t[:, 18], t[:, 19], t[:, 21], t[:, 20], t[:, 13], 1.0 / t[:, 24],
                         mode=mode, iwarm=1)
    n_checked = 0
    for k in range(N_ROWS):
        if t[k, 13] < 1e3:
            continue
        info = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            W.alpha_warm(om, t[k, 18], t[k, 19], t[k, 21], t[k, 20], t[k, 13], 1.0 / t[k, 24], mode, 1, info)
        if not info["converged"]:
            continue
        ar = oplasma.alpha_model(t[k, 0:3], t[k, 3:6], om, mode, 2)
        floor = 1e-9 * 2 * abs(n2[k]) * om / 2.99792458e8 / t[k, 24]
        assert abs(a[k] - ar) <= 1e-7 * (abs(ar) + floor + 1e-300), (k, a[k], ar)
        n_checked += 1
    assert n_checked >= 5
