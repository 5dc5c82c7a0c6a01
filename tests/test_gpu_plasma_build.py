"""torj_plasma_update_gpu, torj_plasma_update_profiles_gpu, torj_plasma_update_device on the GPU:
a live handle whose 2-D spline coefficients are built on the device (torj_coefbuild.hpp) against
a fresh handle of the same plasma, whose coefficients the host built.

Every comparison is array_equal: the device kernels run the host prefilters' IEEE operation
sequences (tests/test_coefbuild_host.py holds their host build to the library's coefficients), so
the coefficients on the device, their lazy download, the cell table k_cell_table rebuilds from
them, and every trace are a fresh handle's bits -- or, on the split path, which reads the rebuilt
table, the bits of a handle brought to the same plasma by the host torj_plasma_update.

Plasmas, rays and helpers: tests/test_gpu_plasma_update.py's (A, B, AB, A2 on 24 x 31 nodes)."""
import ctypes

import numpy as np
import pytest

from test_cell_table_dd import load_harness, run_table
from test_gpu_parity import _compare_trace
from test_gpu_plasma_update import (DS, GRID, KW, N_STEPS, OM, args, eqs, fr, interleaved, rays, same,  # noqa: F401
                                    steps_of, used)
from test_plasma_update_capi import FIELDS, NR, NZ, assert_same, coefs_args, fresh, host_results, with_profiles

pytestmark = pytest.mark.gpu

MAPS = ("psi_norm_data", "Br_data", "Bz_data", "Bphi_data")


def device_maps(eq):
    """eq's four 2-D maps as torch tensors on the GPU, (nZ, nR) contiguous: R fastest"""
    import torch

    dev = torch.device("cuda", 0)
    t = {k: torch.from_numpy(np.ascontiguousarray(np.asarray(eq[k], dtype=np.float64).T)).to(dev) for k in MAPS}
    torch.cuda.synchronize(dev)
    return t


def update_device(P, eq, stream=None):
    t = device_maps(eq)
    P.update_device(eq["R_coords"], eq["Z_coords"], t["psi_norm_data"].data_ptr(), eq["psi_prof"], eq["ne_prof"],
                    eq["Te_prof"], t["Br_data"].data_ptr(), t["Bz_data"].data_ptr(), t["Bphi_data"].data_ptr(),
                    eq["eqt1d_psi_norm"], eq["eqt1d_volume"], stream)
    return t  # (kept alive by the caller until the stream has passed the build)


def profiles(eq):
    return eq["psi_prof"], eq["ne_prof"], eq["Te_prof"]


@pytest.fixture(scope="module")
def points():
    rng = np.random.default_rng(5)
    x = np.stack([rng.uniform(0.7, 3.0, 2000), rng.uniform(-0.3, 0.3, 2000), rng.uniform(-1.1, 1.1, 2000)], 1)
    R = np.hypot(x[:, 0], x[:, 1])
    assert (R < 1.05).any() and (R > 2.65).any() and (np.abs(x[:, 2]) > 0.9).any()  # outside the box too
    return x, rng.standard_normal((2000, 3))


def test_coefficients_and_cell_table(gpu, T, eqs, fr, rays, points):
    import torch

    H = load_harness()
    x, N = points
    P = used(T, eqs["A"], rays["f46", "A"])
    before = P.eval_points(x, N, OM)
    keep = None
    for name, how in (("B", "gpu"), ("A", "gpu"), ("AB", "profiles"), ("A2", "gpu"), ("B", "device")):
        if how == "gpu":
            P.update_gpu(*args(eqs[name]))
        elif how == "profiles":
            P.update_profiles_gpu(*profiles(eqs["B"]))
        else:
            keep = update_device(P, eqs[name])
        F = fr[name]
        got, want = P.eval_points(x, N, OM), F.eval_points(x, N, OM)
        assert np.array_equal(got, want, equal_nan=True), (name, how)
        if name != "A":
            assert not np.array_equal(got, before, equal_nan=True)
        assert P.psi_prof_max == F.psi_prof_max and np.array_equal(P.R_coords, F.R_coords)
        table = P.cell_table()
        hR, hZ = steps_of(F)
        assert np.array_equal(table, run_table(H.ct_record_table, interleaved(F), NR, NZ, hR, hZ)), (name, how)
        for k in FIELDS:  # the lazy download
            assert np.array_equal(P.coefs(k), F.coefs(k)), (name, how, k)
        assert np.array_equal(P.volume(np.linspace(-0.1, 1.3, 29)), F.volume(np.linspace(-0.1, 1.3, 29)))
    torch.cuda.synchronize()
    del keep


@pytest.mark.parametrize("nR,nZ", [(3, 4), (4, 3), (70, 5)])
def test_small_and_odd_grids(gpu, T, points, nR, nZ):
    """no traces here: the point evaluation on the device coefficients, and their download"""
    from torj_hip import synthetic as S

    x, N = points
    a = S.circular_tokamak(nR=nR, nZ=nZ, n_prof=17)
    b = S.circular_tokamak(nR=nR, nZ=nZ, Te0=6000, ne_scale=0.6, n_prof=81, R_range=(1.05, 2.65),
                           Z_range=(-0.85, 0.75))
    P = fresh(T, a)
    P.eval_points(x[:8], N[:8], OM)  # the handle's first GPU use
    keep = None
    for eq, how in ((b, "gpu"), (with_profiles(b, a), "profiles"), (a, "device")):
        if how == "gpu":
            P.update_gpu(*args(eq))
        elif how == "profiles":
            P.update_profiles_gpu(*profiles(a))
        else:
            keep = update_device(P, eq)
        F = fresh(T, eq)
        assert np.array_equal(P.eval_points(x, N, OM), F.eval_points(x, N, OM), equal_nan=True), how
        for k in FIELDS:
            assert np.array_equal(P.coefs(k), F.coefs(k)), (how, k)
    del keep


@pytest.mark.parametrize("lanes", [16, 1])
def test_one_shot_paths(gpu, T, eqs, fr, rays, lanes):
    r = rays["f46", "B"]
    P = used(T, eqs["A"], rays["f46", "A"])
    P.update_gpu(*args(eqs["B"]))
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


def test_split_path(gpu, T, O, eqs, fr, rays):
    """The split pipeline reads the table k_cell_table rebuilds from the device-built coefficients:
    against the CPU oracle of B at test_gpu_parity's bars, and bit for bit a handle brought to B by
    the host torj_plasma_update (k_cell_table on identical coefficients)."""
    r = rays["f130", "B"]
    ds, n = 1e-3, 400
    oa = O.OraclePlasma(*args(eqs["A"])).trace(r["xp"], r["Np"], OM, 1, ds, n)
    ob = O.OraclePlasma(*args(eqs["B"])).trace(r["xp"], r["Np"], OM, 1, ds, n)
    shift = np.abs(oa["state"][:, 6] - ob["state"][:, 6])
    assert shift.min() > 1e-3  # a missed update cannot pass
    P = used(T, eqs["A"], rays["f46", "A"])
    Q = used(T, eqs["A"], rays["f46", "A"])
    P.update_gpu(*args(eqs["B"]))
    Q.update(*args(eqs["B"]))
    try:
        for h in (P, Q):
            h.set_sched(3)
        g = T.trace(P, r["xp"], r["Np"], OM, 1, ds=ds, n_steps=n)
        q = T.trace(Q, r["xp"], r["Np"], OM, 1, ds=ds, n_steps=n)
    finally:
        for h in (P, Q):
            h.set_sched(-1)
    _compare_trace(g, ob)
    same(g, q)


def raw_build(T, P, eq, stream, tensors=None):
    """torj_plasma_update_gpu (tensors: torj_plasma_update_device) on host arrays of this call's own,
    overwritten with NaN as soon as the call has returned"""
    d = T._lib.dptr
    a = [np.array(eq[k], dtype=np.float64) for k in ("R_coords", "Z_coords")]
    a += [np.ascontiguousarray(np.asarray(eq[k], dtype=np.float64).T).copy() for k in MAPS]
    a += [np.array(eq[k], dtype=np.float64) for k in ("psi_prof", "ne_prof", "Te_prof", "eqt1d_psi_norm",
                                                      "eqt1d_volume")]
    R, Z, psi, Br, Bz, Bp, pp, ne, te, ep, ev = a
    if tensors is None:
        T._lib.check(T.lib().torj_plasma_update_gpu(P.handle, d(R), d(Z), d(psi), len(pp), d(pp), d(ne), d(te), d(Br),
                                                    d(Bz), d(Bp), len(ep), d(ep), d(ev), stream))
    else:
        m = [tensors[k].data_ptr() for k in MAPS]
        T._lib.check(T.lib().torj_plasma_update_device(P.handle, d(R), d(Z), m[0], len(pp), d(pp), d(ne), d(te), m[1],
                                                       m[2], m[3], len(ep), d(ep), d(ev), stream))
    for v in a:
        v.fill(np.nan)


@pytest.mark.parametrize("how", ["stream", "null", "device"])
def test_stream_order(gpu, T, eqs, fr, rays, how):
    """build(A), trace, build(B), trace on one stream with no synchronisation in between"""
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
    maps = {k: device_maps(eqs[k]) if how == "device" else None for k in ("A", "B")}
    torch.cuda.synchronize(dev)
    st = torch.cuda.current_stream(dev) if how == "null" else torch.cuda.Stream(dev)
    s = ctypes.c_void_p(st.cuda_stream)
    assert bool(s.value) != (how == "null")
    L = T.lib()
    for name, b in (("A", bufs[0]), ("B", bufs[1])):
        raw_build(T, P, eqs[name], s, maps[name])
        T._lib.check(L.torj_trace_device_ex(P.handle, cfg, n, b["x0"].data_ptr(), b["N0"].data_ptr(), None, 0, None,
                                            None, None, b["state"].data_ptr(), b["status"].data_ptr(),
                                            b["steps"].data_ptr(), None, None, None, None, s))
    T._lib.check(L.torj_trace_check(P.handle, s))
    if how == "device":  # the stream has been synchronised: the maps may go
        for m in maps.values():
            for v in m.values():
                v.fill_(float("nan"))
    for name, r, b in (("A", rA, bufs[0]), ("B", rB, bufs[1])):
        want = T.trace(fr[name], r["xp"], r["Np"], OM, 1, **KW)
        assert np.array_equal(b["state"].cpu().numpy().T, want.state), name
        assert np.array_equal(b["status"].cpu().numpy(), want.status), name
        assert np.array_equal(b["steps"].cpu().numpy(), want.steps), name
        assert (want.steps > 0).all()


@pytest.fixture(scope="module")
def want_host(T, eqs):
    """fresh handles' host results, computed once"""
    return {k: host_results(T, fresh(T, eqs[k])) for k in ("A", "B", "AB")}


def test_host_mirror(gpu, T, eqs, fr, rays, want_host):
    r = rays["f46", "AB"]
    P = used(T, eqs["A"], rays["f46", "A"])
    P.update_gpu(*args(eqs["B"]))
    assert_same(host_results(T, P), want_host["B"])
    # the host update_profiles after update_device: both the coefficients and the psi nodes come down
    keep = update_device(P, eqs["A"])
    P.update_profiles(*profiles(eqs["B"]))
    assert_same(host_results(T, P), want_host["AB"])
    same(T.trace(P, r["xp"], r["Np"], OM, 1, **KW), T.trace(fr["AB"], r["xp"], r["Np"], OM, 1, **KW))
    del keep
    # a host update after a GPU update replaces the mirror
    P.update_gpu(*args(eqs["B"]))
    P.update(*args(eqs["A"]))
    assert_same(host_results(T, P), want_host["A"])
    rA, rB = rays["f46", "A"], rays["f46", "B"]
    same(T.trace(P, rA["xp"], rA["Np"], OM, 1, **KW), T.trace(fr["A"], rA["xp"], rA["Np"], OM, 1, **KW))
    # ... and a GPU update after a host update
    P.update(*args(eqs["A2"]))
    P.update_gpu(*args(eqs["B"]))
    same(T.trace(P, rB["xp"], rB["Np"], OM, 1, **KW), T.trace(fr["B"], rB["xp"], rB["Np"], OM, 1, **KW))
    assert_same(host_results(T, P), want_host["B"])
    # profiles on the device after a host update: the psi nodes go up on first need
    P.update(*args(eqs["A"]))
    P.update_profiles_gpu(*profiles(eqs["B"]))
    assert_same(host_results(T, P), want_host["AB"])


def test_first_gpu_use(gpu, T, eqs, fr, rays):
    """update_gpu on a handle never used on the GPU: it gets its device state first"""
    r = rays["f46", "B"]
    P = fresh(T, eqs["A"])
    P.update_gpu(*args(eqs["B"]))
    same(T.trace(P, r["xp"], r["Np"], OM, 1, **KW), T.trace(fr["B"], r["xp"], r["Np"], OM, 1, **KW))
    Q = fresh(T, eqs["A"])
    Q.update_profiles_gpu(*profiles(eqs["B"]))
    r = rays["f46", "AB"]
    same(T.trace(Q, r["xp"], r["Np"], OM, 1, **KW), T.trace(fr["AB"], r["xp"], r["Np"], OM, 1, **KW))


def test_profiles_on_a_from_coefs_handle_refused(gpu, T, eqs, fr, rays):
    r = rays["f46", "A"]
    P = T.Plasma.from_coefs(*coefs_args(T, eqs["A"]))
    a = T.trace(P, r["xp"], r["Np"], OM, 1, **KW)
    with pytest.raises(T.TorjError, match="torj_plasma_update_profiles_gpu: the handle has no psi_norm_data"):
        P.update_profiles_gpu(*profiles(eqs["B"]))
    same(T.trace(P, r["xp"], r["Np"], OM, 1, **KW), a)
    same(a, T.trace(fr["A"], r["xp"], r["Np"], OM, 1, **KW))
    # ... and after update_device, which leaves the psi nodes on the device, it goes through
    keep = update_device(P, eqs["A"])
    P.update_profiles_gpu(*profiles(eqs["B"]))
    r = rays["f46", "AB"]
    same(T.trace(P, r["xp"], r["Np"], OM, 1, **KW), T.trace(fr["AB"], r["xp"], r["Np"], OM, 1, **KW))
    del keep


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
        P.update_gpu(*args(eqs["B"]))
        a = T.trace(P, rB["xp"], rB["Np"], OM, 1, **KW, **depo(rB))  # the same workspaces, no error
        c, t2, p2 = read()
        assert c == 1 and t2 > 0 and p2 > 0  # timing is still on
        same(a, T.trace(F, rB["xp"], rB["Np"], OM, 1, **KW, **depo(rB)))  # one lane per ray still
    finally:
        T._lib.check(L.torj_timing(P.handle, 0))
        for h in (P, F):
            h.set_sched(-1)


def test_multi_plasma_pool(gpu, T, eqs, fr, rays):
    """three pooled handles refilled by the three calls, one launch through them against one launch
    per beam on fresh handles"""
    names = ("B", "AB", "A2")
    pool = [used(T, eqs["A"], rays["f46", "A"]) for _ in names]
    pool[0].update_gpu(*args(eqs["B"]))
    pool[1].update_profiles_gpu(*profiles(eqs["B"]))
    keep = update_device(pool[2], eqs["A2"])
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
        assert len({m.state[k].tobytes() for k in (0, 5, 6)}) == 3
    finally:
        for h in every:
            h.set_sched(-1)
    del keep


def test_replicas_follow(gpu, T, eqs, fr, rays, monkeypatch):
    """torj_trace_beam over two replicas (both on device 0), update_gpu, torj_trace_beam again: the
    replica takes the built coefficients by a device copy"""
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
        P.update_gpu(*args(eqs["B"]))
        T._lib.check(L.torj_timing(P.handle, 1))
        a = T.trace(P, rB["xp"], rB["Np"], OM, 1, **kw(rB))
        calls, t_tr = (ctypes.c_int * 2)(), (ctypes.c_double * 2)()
        T._lib.check(L.torj_beam_timing_read(P.handle, 2, calls, t_tr, None, None))
        T._lib.check(L.torj_timing(P.handle, 0))
        assert list(calls) == [1, 1] and all(v > 0 for v in t_tr)  # both replicas traced their shard
        b = T.trace(F, rB["xp"], rB["Np"], OM, 1, **kw(rB))
        # replicas made after a device-side build: from the downloaded mirror
        Q = used(T, eqs["A"], rays["f46", "A"])
        Q.set_sched(0)
        Q.update_gpu(*args(eqs["B"]))
        c = T.trace(Q, rB["xp"], rB["Np"], OM, 1, **kw(rB))
    finally:
        for h in (P, F):
            h.set_sched(-1)
    for got in (a, c):
        for f in ("state", "status", "steps", "P_dep"):
            assert np.array_equal(getattr(got, f), getattr(b, f)), f
        assert np.array_equal(got.traj, b.traj, equal_nan=True)
        assert np.abs(got.dP_shell - b.dP_shell).max() <= 1e-13 * np.abs(b.dP_shell).max()
    assert b.dP_shell[-1] > 0
