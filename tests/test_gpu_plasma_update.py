"""torj_plasma_update, torj_plasma_update_profiles, torj_plasma_get_cell_table on the GPU:
a live handle updated to a plasma against a fresh handle of that plasma.

The coefficients on the device, the one-shot / adaptive / multi-beam traces, the stream
order of update and trace, the replicas of torj_trace_beam and the handle's settings are
held bit for bit; the cell table, rebuilt by k_cell_table, is held array_equal to the
host run of the same record function (tests/native/cell_table_host.hip, whose arithmetic
tests/test_cell_table_dd.py holds against exact rationals) and within 1 ulp + 2^-58 S of a
fresh handle's long double table; the split pipeline, which alone reads that table, is
held to the CPU oracle at test_gpu_parity's bars.

Plasmas: tests/test_plasma_update_capi.py's A and B on 24 x 31 nodes, A with B's profiles,
and A on another box.  Rays: SETUP's launch point; beams of 5, 1 and 13 rays, the 46-ray
fan, 130 rays (two full 64-ray groups and a partial one) for the split path and the
replicas."""
import ctypes

import numpy as np
import pytest

from test_cell_table_dd import M6, NF, load_harness, run_table
from test_gpu_parity import _compare_trace
from test_plasma_update_capi import FIELDS, NR, NZ, fresh, tokamak_a, tokamak_b, with_profiles

pytestmark = pytest.mark.gpu

OM = 2 * np.pi * 92.5e9
DS, N_STEPS = 5e-4, 600  # 30 cm: through the X2 resonance
KW = dict(ds=DS, n_steps=N_STEPS)
GRID = np.linspace(0.0, 1.0, 60)
SLOT = dict(Br=0, Bphi=1, Bz=2, lnne=3, lnTe=4, psi=5)  # torj_math.hpp Field


def args(eq):
    from torj_hip import synthetic as S

    return S.plasma_args(eq)


@pytest.fixture(scope="module")
def eqs():
    from torj_hip import synthetic as S

    A, B = tokamak_a(), tokamak_b()
    A2 = S.circular_tokamak(nR=NR, nZ=NZ, R_range=(0.95, 2.7), Z_range=(-0.9, 0.82))
    return dict(A=A, B=B, AB=with_profiles(A, B), A2=A2)


@pytest.fixture(scope="module")
def fr(T, eqs):
    """one fresh handle per plasma, shared (never updated)"""
    return {k: fresh(T, eq) for k, eq in eqs.items()}


def fan(T, n_rings=3):
    from torj_hip import synthetic as S

    s = S.SETUP
    N0 = T.pol_tor_angles_2_vector(s["steering_angle_pol"], s["steering_angle_tor"])
    return T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"], s["inverse_curvature_radius"],
                                    s["f_abs_test"], N_rings=n_rings)


@pytest.fixture(scope="module")
def rays(T, fr):
    """launch and entry states (host entry, no GPU use): the 46-ray fan and 130 rays of the
    8-ring fan, entered into each plasma"""
    out = {}
    for name, (pos, dirs, w) in (("f46", fan(T)), ("f130", tuple(a[:130] for a in fan(T, 8)))):
        for k, P in fr.items():
            xp, Np, s0, st = T.ray_entry(P, pos, dirs, OM, 1)
            assert (st == 0).all()
            out[name, k] = dict(pos=pos, w=w, xp=xp, Np=Np, s0=s0)
    assert len(out["f46", "A"]["w"]) == 46 and len(out["f130", "A"]["w"]) == 130
    return out


def used(T, eq, r):
    """a handle of eq whose device state exists: traced once"""
    P = fresh(T, eq)
    T.trace(P, r["xp"][:5], r["Np"][:5], OM, 1, ds=DS, n_steps=20)
    return P


def same(a, b):
    for f in ("state", "status", "steps", "P_dep", "dP_shell"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.traj is None) == (b.traj is None)
    if a.traj is not None:
        assert np.array_equal(a.traj, b.traj, equal_nan=True)


def interleaved(P):
    """the handle's node coefficients as the library keeps them: (nZ + 2, nR + 2, NF)"""
    c = np.zeros((NZ + 2, NR + 2, NF))
    for k in FIELDS:
        c[..., SLOT[k]] = P.coefs(k).T
    return c


def steps_of(P):
    R, Z = P.R_coords, P.Z_coords
    return (R[-1] - R[0]) / (NR - 1), (Z[-1] - Z[0]) / (NZ - 1)


def test_coefficients_on_the_device(gpu, T, eqs, fr, rays):
    P = used(T, eqs["A"], rays["f46", "A"])
    rng = np.random.default_rng(5)
    x = np.stack([rng.uniform(0.7, 3.0, 2000), rng.uniform(-0.3, 0.3, 2000), rng.uniform(-1.1, 1.1, 2000)], 1)
    R = np.hypot(x[:, 0], x[:, 1])
    assert (R < 1.05).any() and (R > 2.65).any() and (np.abs(x[:, 2]) > 0.9).any()  # outside the box too
    N = rng.standard_normal((2000, 3))
    before = P.eval_points(x, N, OM)
    P.update(*args(eqs["B"]))
    got, want = P.eval_points(x, N, OM), fr["B"].eval_points(x, N, OM)
    assert np.array_equal(got, want, equal_nan=True)
    assert not np.array_equal(got, before, equal_nan=True)


def table_S(coef, hR, hZ):
    """S = sum |M_jb M_ia c_ba| / (36 hR^i hZ^j) per entry of the table, (nZ - 1, nR - 1, 6, 4, 4)"""
    M = np.abs(np.array(M6, dtype=np.float64))
    a = np.abs(coef[..., :6])
    win = np.stack([np.stack([a[b:b + NZ - 1, k:k + NR - 1] for k in range(4)], -1) for b in range(4)], -2)
    S = np.einsum("jb,ia,zrfba->zrfji", M, M, win) / 36.0  # win: (z, r, f, b, a)
    return S / (hR ** np.arange(4))[None, None, None, None, :] / (hZ ** np.arange(4))[None, None, None, :, None]


def test_cell_table(gpu, T, eqs, fr, rays):
    H = load_harness()
    r = rays["f46", "A"]
    P = used(T, eqs["A"], r)
    t_a = P.cell_table()
    P.update(*args(eqs["B"]))
    got = P.cell_table()
    hR, hZ = steps_of(fr["B"])
    coef = interleaved(fr["B"])
    # the kernel's table: the host run of the same record function, bit for bit
    assert np.array_equal(got, run_table(H.ct_record_table, coef, NR, NZ, hR, hZ))
    assert not np.array_equal(got, t_a)
    # a fresh handle's table (cell_power_table, long double, on its first GPU use)
    T.trace(fr["B"], r["xp"][:5], r["Np"][:5], OM, 1, ds=DS, n_steps=20)
    want = fr["B"].cell_table()
    assert np.array_equal(want, run_table(H.ct_host_table, coef, NR, NZ, hR, hZ))
    ulp = np.spacing(np.minimum(np.abs(got), np.abs(want)))
    d = np.abs(got - want)
    bar = ulp + 2.0 ** -58 * table_S(coef, hR, hZ)
    print(f"updated vs fresh cell table: {np.count_nonzero(d)} of {d.size} entries differ, "
          f"max |d| / bar {np.max(d / np.where(bar > 0, bar, 1.0)):.3f}")
    assert (d <= bar).all()
    # updated before its first GPU use: host-only, in every bit a fresh handle
    Q = fresh(T, eqs["A"])
    Q.update(*args(eqs["B"]))
    T.trace(Q, r["xp"][:5], r["Np"][:5], OM, 1, ds=DS, n_steps=20)
    assert np.array_equal(Q.cell_table(), want)


@pytest.mark.parametrize("lanes", [16, 1])
def test_one_shot_paths(gpu, T, eqs, fr, rays, lanes):
    r = rays["f46", "B"]
    P = used(T, eqs["A"], rays["f46", "A"])
    P.update(*args(eqs["B"]))
    F = fr["B"]
    depo = dict(psi_grid=GRID, weights=r["w"], deposition="reference", x_launch=r["pos"], s0=r["s0"], traj_stride=50)
    try:
        for h in (P, F):
            h.set_sched(2 if lanes == 16 else 0)
        for kw in ({}, depo):
            a, b = (T.trace(h, r["xp"], r["Np"], OM, 1, **KW, **kw) for h in (P, F))
            same(a, b)
            assert (a.steps > 0).all()
        assert a.dP_shell[:-2].any()
    finally:
        for h in (P, F):
            h.set_sched(-1)
    if lanes == 16:  # the adaptive integrator (the work-queue kernel), 3 rays
        kw = dict(ds=1e-4, n_steps=3000, integrator="adaptive", s_max=0.3, psi_grid=GRID, weights=r["w"][:3],
                  deposition="reference", x_launch=r["pos"][:3], s0=r["s0"][:3], traj_stride=1)
        a, b = (T.trace(h, r["xp"][:3], r["Np"][:3], OM, 1, **kw) for h in (P, F))
        same(a, b)
        assert (a.steps > 10).all()


def test_multi_plasma_pool(gpu, T, eqs, fr, rays):
    """three pooled handles refilled, one launch through them against one launch per beam on
    fresh handles"""
    names = ("B", "AB", "A2")
    pool = [used(T, eqs["A"], rays["f46", "A"]) for _ in names]
    pool[0].update(*args(eqs["B"]))
    pool[1].update_profiles(eqs["B"]["psi_prof"], eqs["B"]["ne_prof"], eqs["B"]["Te_prof"])
    pool[2].update(*args(eqs["A2"]))
    counts, bp = (5, 1, 13, 46), (0, 1, 2, 1)
    off = np.concatenate([[0], np.cumsum(counts)])
    cat = {k: np.concatenate([rays["f46", names[j]][k][:c] for c, j in zip(counts, bp)])
           for k in ("pos", "w", "xp", "Np", "s0")}
    depo = lambda d, sl=slice(None): dict(psi_grid=GRID, weights=d["w"][sl], deposition="reference",
                                          x_launch=d["pos"][sl], s0=d["s0"][sl], traj_stride=100)
    every = pool + [fr[k] for k in names]
    try:
        for h in every:
            h.set_sched(2)
        m = T.trace_beams(pool[0], off, [OM] * 4, [1] * 4, cat["xp"], cat["Np"], **KW, **depo(cat), plasmas=pool,
                          beam_plasma=list(bp))
        for b, (c, j) in enumerate(zip(counts, bp)):
            sl = slice(off[b], off[b + 1])
            s = T.trace(fr[names[j]], cat["xp"][sl], cat["Np"][sl], OM, 1, **KW, **depo(cat, sl))
            for f in ("state", "status", "steps", "P_dep"):
                assert np.array_equal(getattr(m, f)[sl], getattr(s, f)), (b, f)
            assert np.array_equal(m.traj[sl], s.traj, equal_nan=True)
            assert np.array_equal(m.dP_shell[b], s.dP_shell)
        # ray 0 of the fan through B, AB and A2 (beams 0, 1, 2) ends in three places
        assert len({m.state[k].tobytes() for k in (0, 5, 6)}) == 3
    finally:
        for h in every:
            h.set_sched(-1)


def test_split_path_parity(gpu, T, O, eqs, fr, rays):
    """The split pipeline reads the rebuilt table: 130 rays, 400 steps of 1 mm, Albajar,
    against the CPU oracle of B at test_gpu_parity's bars.

    The direct difference between the updated and the fresh handle is printed, with no bar on
    it: 2.2e-16 in x and N, 5.3e-15 in tau on an MI355X (profiles/r15/pytest_gpu.txt,
    DESIGN.md 3.2e)."""
    r = rays["f130", "B"]
    ds, n = 1e-3, 400
    oa = O.OraclePlasma(*args(eqs["A"])).trace(r["xp"], r["Np"], OM, 1, ds, n)
    ob = O.OraclePlasma(*args(eqs["B"])).trace(r["xp"], r["Np"], OM, 1, ds, n)
    # a missed update cannot pass: the same rays through A end elsewhere in tau
    shift = np.abs(oa["state"][:, 6] - ob["state"][:, 6])
    print(f"oracle tau shift A vs B: max {shift.max():.3e}, min {shift.min():.3e}")
    assert shift.min() > 1e-3
    P = used(T, eqs["A"], rays["f46", "A"])
    P.update(*args(eqs["B"]))
    F = fr["B"]
    try:
        for h in (P, F):
            h.set_sched(3)
        g = T.trace(P, r["xp"], r["Np"], OM, 1, ds=ds, n_steps=n)
        f = T.trace(F, r["xp"], r["Np"], OM, 1, ds=ds, n_steps=n)
    finally:
        for h in (P, F):
            h.set_sched(-1)
    _compare_trace(g, ob)
    _compare_trace(f, ob)
    assert np.array_equal(g.status, f.status) and np.array_equal(g.steps, f.steps)
    dx = np.abs(g.state[:, :6] - f.state[:, :6]).max()
    dt = np.abs(g.state[:, 6] - f.state[:, 6])
    print(f"split path, updated vs fresh handle: max |d x, N| {dx:.3e}, max |d tau| {dt.max():.3e} "
          f"(relative {np.max(dt / np.maximum(np.abs(f.state[:, 6]), 1e-6)):.3e})")


def raw_update(T, P, eq, stream):
    """torj_plasma_update on arrays of this call's own, overwritten with NaN as soon as the
    call has returned"""
    d = T._lib.dptr
    a = [np.array(eq[k], dtype=np.float64) for k in ("R_coords", "Z_coords")]
    a += [np.ascontiguousarray(np.asarray(eq[k], dtype=np.float64).T).copy()
          for k in ("psi_norm_data", "Br_data", "Bz_data", "Bphi_data")]
    a += [np.array(eq[k], dtype=np.float64) for k in ("psi_prof", "ne_prof", "Te_prof", "eqt1d_psi_norm",
                                                      "eqt1d_volume")]
    R, Z, psi, Br, Bz, Bp, pp, ne, te, ep, ev = a
    T._lib.check(T.lib().torj_plasma_update(P.handle, d(R), d(Z), d(psi), len(pp), d(pp), d(ne), d(te), d(Br),
                                            d(Bz), d(Bp), len(ep), d(ep), d(ev), stream))
    for v in a:
        v.fill(np.nan)


@pytest.mark.parametrize("null_stream", [False, True], ids=["stream", "null"])
def test_stream_order(gpu, T, eqs, fr, rays, null_stream):
    """update(A), trace, update(B), trace on one stream with no synchronisation in between"""
    import torch

    dev = torch.device("cuda", 0)
    P = used(T, eqs["A2"], rays["f46", "A2"])
    rA, rB = rays["f46", "A"], rays["f46", "B"]
    n = 46
    cfg = T._lib.TraceCfg(OM, 1, DS, N_STEPS, N_STEPS // 100, 1.0, 1e-6, 1, 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    bufs = []
    for r in (rA, rB):
        bufs.append(dict(x0=t(r["xp"].T), N0=t(r["Np"].T), state=torch.zeros((7, n), dtype=torch.float64, device=dev),
                         status=torch.full((n,), -1, dtype=torch.int32, device=dev),
                         steps=torch.full((n,), -1, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize(dev)
    st = torch.cuda.current_stream(dev) if null_stream else torch.cuda.Stream(dev)
    s = ctypes.c_void_p(st.cuda_stream)
    assert bool(s.value) != null_stream
    L = T.lib()
    for eq, b in ((eqs["A"], bufs[0]), (eqs["B"], bufs[1])):
        raw_update(T, P, eq, s)
        T._lib.check(L.torj_trace_device_ex(P.handle, cfg, n, b["x0"].data_ptr(), b["N0"].data_ptr(), None, 0, None,
                                            None, None, b["state"].data_ptr(), b["status"].data_ptr(),
                                            b["steps"].data_ptr(), None, None, None, None, s))
    T._lib.check(L.torj_trace_check(P.handle, s))
    for name, r, b in (("A", rA, bufs[0]), ("B", rB, bufs[1])):
        want = T.trace(fr[name], r["xp"], r["Np"], OM, 1, **KW)
        assert np.array_equal(b["state"].cpu().numpy().T, want.state), name
        assert np.array_equal(b["status"].cpu().numpy(), want.status), name
        assert np.array_equal(b["steps"].cpu().numpy(), want.steps), name
        assert (want.steps > 0).all()


def test_replicas_follow(gpu, T, eqs, fr, rays, monkeypatch):
    """torj_trace_beam over two replicas (both on device 0), update, torj_trace_beam again"""
    monkeypatch.setenv("TORJ_BEAM_SAME_DEVICE", "1")
    rA, rB = rays["f130", "A"], rays["f130", "B"]
    kw = lambda r: dict(ds=1e-4, n_steps=12000, psi_grid=np.linspace(0, 1, 200), weights=r["w"], traj_stride=1000,
                        deposition="reference", x_launch=r["pos"], s0=r["s0"], n_gpus=2)
    P, F = fresh(T, eqs["A"]), fr["B"]
    L = T.lib()
    try:
        for h in (P, F):
            h.set_sched(0)
        T.trace(P, rA["xp"], rA["Np"], OM, 1, **kw(rA))  # the replica exists and has traced
        P.update(*args(eqs["B"]))
        T._lib.check(L.torj_timing(P.handle, 1))
        a = T.trace(P, rB["xp"], rB["Np"], OM, 1, **kw(rB))
        calls, t_tr = (ctypes.c_int * 2)(), (ctypes.c_double * 2)()
        T._lib.check(L.torj_beam_timing_read(P.handle, 2, calls, t_tr, None, None))
        T._lib.check(L.torj_timing(P.handle, 0))
        assert list(calls) == [1, 1] and all(v > 0 for v in t_tr)  # both replicas traced their shard
        b = T.trace(F, rB["xp"], rB["Np"], OM, 1, **kw(rB))
    finally:
        for h in (P, F):
            h.set_sched(-1)
    for f in ("state", "status", "steps", "P_dep"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.traj, b.traj, equal_nan=True)
    assert b.dP_shell[-1] > 0
    assert np.abs(a.dP_shell - b.dP_shell).max() <= 1e-13 * np.abs(b.dP_shell).max()


def test_settings_and_workspaces_survive(gpu, T, eqs, fr, rays):
    rA, rB = rays["f46", "A"], rays["f46", "B"]
    depo = lambda r: dict(psi_grid=GRID, weights=r["w"], deposition="reference", x_launch=r["pos"], s0=r["s0"])
    P, F = fresh(T, eqs["A"]), fr["B"]
    L = T.lib()

    def read():
        calls, t_tr, t_po = ctypes.c_int(-1), ctypes.c_double(-1), ctypes.c_double(-1)
        T._lib.check(L.torj_timing_read(P.handle, ctypes.byref(calls), ctypes.byref(t_tr), ctypes.byref(t_po)))
        return calls.value, t_tr.value, t_po.value

    try:
        for h in (P, F):
            h.set_sched(0)
        T._lib.check(L.torj_timing(P.handle, 1))
        T.trace(P, rA["xp"], rA["Np"], OM, 1, **KW, **depo(rA))
        c, t1, p1 = read()
        assert c == 1 and t1 > 0 and p1 > 0
        P.update(*args(eqs["B"]))
        a = T.trace(P, rB["xp"], rB["Np"], OM, 1, **KW, **depo(rB))  # the same workspaces, no error
        c, t2, p2 = read()
        assert c == 1 and t2 > 0 and p2 > 0  # timing is still on
        same(a, T.trace(F, rB["xp"], rB["Np"], OM, 1, **KW, **depo(rB)))  # one lane per ray still: the fresh
        # handle's bits at that setting
    finally:
        T._lib.check(L.torj_timing(P.handle, 0))
        for h in (P, F):
            h.set_sched(-1)
