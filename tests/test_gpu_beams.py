"""Many small beams of differing frequency and mode in one launch
(torj_trace_beams[_device], torj_ray_entry_beams_gpu, make_beams) on the GPU:
bit-identical to one launch per beam with the same lanes per ray, and each beam
against the CPU oracle with its own frequency and mode.

Workload: the synthetic tokamak and SETUP's launch point, the default 46-ray
fan per beam, 12 000 steps of 1e-4 m with termination checks every 120 --
long enough that rays of one beam end OK, LEFT_PLASMA and ABSORBED -- on 200
shell boundaries, trajectory samples every 1 000 steps.  Six beams, 111 rays:
46 + 5 + 0 + 1 + 46 + 13, so that beams end inside a wave at both 4 and 64 rays
per wave, one is empty and one is a single ray."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import _compare_trace

pytestmark = pytest.mark.gpu

DS, N_STEPS, CHUNK, STRIDE = 1e-4, 12000, 120, 1000
GRID = np.linspace(0.0, 1.0, 200)
# frequency, mode, steering pol / tor (degrees), rays taken from the 46-ray fan
BEAMS = (
    (92.5e9, 1, 30.0, 0.0, 46),
    (92.5e9, -1, 30.0, 0.0, 5),
    (140e9, 1, 30.0, 0.0, 0),
    (110e9, 1, 30.0, 0.0, 1),
    (100e9, 1, 35.0, -5.0, 46),
    (85.5e9, -1, 25.0, 5.0, 13),
)


def fan(T, f, pol, tor):
    from torj_hip import synthetic as S

    s = S.SETUP
    N0 = T.pol_tor_angles_2_vector(np.deg2rad(pol), np.deg2rad(tor))
    return T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"],
                                    s["inverse_curvature_radius"], f)


@pytest.fixture(scope="module")
def beams(T, hplasma):
    """The six beams' concatenated launch and entry states and their tables."""
    pos, dirs, w, xp, Np, s0, off, omega, mode = [], [], [], [], [], [], [0], [], []
    for f, m, pol, tor, k in BEAMS:
        p, d, ww = fan(T, f, pol, tor)
        assert len(ww) == 46
        om = 2 * np.pi * f
        x, N, s, st = T.ray_entry(hplasma, p, d, om, m)
        assert (st == 0).all()
        for lst, a in ((pos, p), (dirs, d), (w, ww), (xp, x), (Np, N), (s0, s)):
            lst.append(a[:k])
        off.append(off[-1] + k)
        omega.append(om)
        mode.append(m)
    cat = {k: np.concatenate(v) for k, v in dict(pos=pos, dirs=dirs, w=w, xp=xp, Np=Np, s0=s0).items()}
    assert off == [0, 46, 51, 51, 52, 98, 111]
    return dict(off=off, omega=omega, mode=mode, **cat)


KW = dict(ds=DS, n_steps=N_STEPS, chunk_steps=CHUNK, traj_stride=STRIDE)


def depo_kw(b, deposition, sl=slice(None)):
    if deposition == "none":
        return {}
    kw = dict(psi_grid=GRID, weights=b["w"][sl], deposition=deposition)
    if deposition == "reference":
        kw.update(x_launch=b["pos"][sl], s0=b["s0"][sl])
    return kw


def single(T, hplasma, b, k, deposition):
    """beam k alone: one T.trace"""
    sl = slice(b["off"][k], b["off"][k + 1])
    return sl, T.trace(hplasma, b["xp"][sl], b["Np"][sl], b["omega"][k], b["mode"][k], **KW,
                       **depo_kw(b, deposition, sl))


def per_ray_equal(m, sl, s):
    assert np.array_equal(m.state[sl], s.state)
    assert np.array_equal(m.status[sl], s.status)
    assert np.array_equal(m.steps[sl], s.steps)
    assert np.array_equal(m.P_dep[sl], s.P_dep)
    assert np.array_equal(m.traj[sl], s.traj, equal_nan=True)


@pytest.mark.parametrize("deposition", ["none", "reference"])
@pytest.mark.parametrize("lanes", [16, 1])
def test_beams_equal_single_launches(gpu, T, hplasma, beams, lanes, deposition):
    """One multi-beam launch against one launch per beam with the same lanes per ray:
    a wave of the multi-beam launch holds the rays it holds in the beam's own launch,
    so every output is the same bits (the 16-lane Albajar code chooses per wave)."""
    b = beams
    try:
        hplasma.set_sched(2 if lanes == 16 else 0)
        m = T.trace_beams(hplasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], **KW,
                          **depo_kw(b, deposition))
        assert m.dP_shell.shape == (6, len(GRID) + 1 if deposition != "none" else 1)
        for k in range(6):
            if b["off"][k] == b["off"][k + 1]:
                assert not m.dP_shell[k].any()  # the empty beam's row
                continue
            sl, s = single(T, hplasma, b, k, deposition)
            per_ray_equal(m, sl, s)
            if deposition == "reference":
                assert np.array_equal(m.dP_shell[k], s.dP_shell)
        if deposition == "reference":
            assert m.dP_shell[:, :-2].any()
    finally:
        hplasma.set_sched(-1)


def test_beams_binned_equal_single_launches(gpu, T, hplasma, beams):
    """Binned deposition (one lane per ray): per-ray outputs the same bits, the shells'
    atomic sums to their order -- the bar of test_device_pointer_trace_async_grid_check."""
    b = beams
    try:
        hplasma.set_sched(0)
        m = T.trace_beams(hplasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], **KW, **depo_kw(b, "binned"))
        for k in range(6):
            if b["off"][k] == b["off"][k + 1]:
                assert not m.dP_shell[k].any()
                continue
            sl, s = single(T, hplasma, b, k, "binned")
            per_ray_equal(m, sl, s)
            err = np.abs(m.dP_shell[k] - s.dP_shell).max()
            print(f"beam {k}: dP row differs by {err:.3e} of max {np.abs(s.dP_shell).max():.3e}")
            assert err <= 1e-12 * np.abs(s.dP_shell).max()
    finally:
        hplasma.set_sched(-1)


class _Beam:
    """rays sl of a multi-beam TraceResult as _compare_trace reads them"""

    def __init__(self, m, sl):
        self.state, self.status, self.steps = m.state[sl], m.status[sl], m.steps[sl]


def test_beams_match_oracle(gpu, T, hplasma, oplasma, beams):
    """The automatic path with binned deposition, each beam against the oracle traced
    with that beam's own frequency and mode, at test_gpu_parity's bars.  (A launch
    with one frequency for all rays cannot pass this.)"""
    b = beams
    m = T.trace_beams(hplasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], **KW, **depo_kw(b, "binned"))
    seen = set()
    for k in range(6):
        sl = slice(b["off"][k], b["off"][k + 1])
        if sl.start == sl.stop:
            continue
        o = oplasma.trace(b["xp"][sl], b["Np"][sl], b["omega"][k], b["mode"][k], DS, N_STEPS, chunk_steps=CHUNK,
                          psi_grid=GRID, weights=b["w"][sl])
        seen |= set(o["status"].tolist())
        _compare_trace(_Beam(m, sl), o)
        scale = max(np.abs(o["dP"]).max(), 1e-300)
        err = np.abs(m.dP_shell[k, :-1] - o["dP"]).max()
        print(f"beam {k}: dP differs from the oracle's by {err:.3e} of max {scale:.3e}")
        assert err <= 1e-10 * scale
        assert np.abs(m.P_dep[sl] - o["Pdep"]).max() <= 1e-10 * max(o["Pdep"].max(), 1e-300)
    # all three ends occur in the oracle's own results (else the workload is too short)
    assert {T.OK, T.LEFT_PLASMA, T.ABSORBED} <= seen


def test_beams_device_back_to_back(gpu, T, hplasma, beams):
    """Two torj_trace_beams_device calls on one stream with no sync between them, the
    host tables overwritten with the second call's values as soon as the first has
    returned, then one torj_trace_check: each call saw its own tables.  The counters
    are the sums over the beams; a non-increasing grid is found on the device."""
    import torch

    b = beams
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    L = T.lib()
    cfg = T._lib.TraceCfg(0.0, 0, DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, 0)
    sets = ((0, 4), (4, 6))  # beams 0..3 (52 rays), beams 4..5 (59 rays)

    def t(a, dtype=torch.float64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dtype)

    def tables(lo, hi):
        off = np.array(b["off"][lo:hi + 1], dtype=np.int32) - b["off"][lo]
        return off, np.array(b["omega"][lo:hi]), np.array(b["mode"][lo:hi], dtype=np.int32)

    class Call:
        def __init__(self, lo, hi, grid=None):
            sl = slice(b["off"][lo], b["off"][hi])
            self.n, self.nb = sl.stop - sl.start, hi - lo
            self.x0, self.N0 = t(b["xp"][sl].T), t(b["Np"][sl].T)
            self.state = torch.empty((7, self.n), dtype=torch.float64, device=dev)
            self.status = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.steps = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.counters = torch.zeros(8, dtype=torch.int64, device=dev)
            self.grid = t(grid) if grid is not None else None
            self.w = t(b["w"][sl]) if grid is not None else None
            self.dP = torch.zeros((self.nb, len(grid) + 1), dtype=torch.float64, device=dev) if grid is not None else None

        def enqueue(self, off, om, md):
            g = self.grid
            T._lib.check(L.torj_trace_beams_device(
                hplasma.handle, cfg, self.nb, T._lib.iptr(off), T._lib.dptr(om), T._lib.iptr(md),
                self.x0.data_ptr(), self.N0.data_ptr(), self.w.data_ptr() if g is not None else None,
                len(g) if g is not None else 0, g.data_ptr() if g is not None else None, None, None,
                self.state.data_ptr(), self.status.data_ptr(), self.steps.data_ptr(),
                self.dP.data_ptr() if g is not None else None, None, None, self.counters.data_ptr(),
                stream.cuda_stream))

        def out(self):
            return [a.cpu().numpy() for a in (self.state, self.status, self.steps, self.counters)]

    # separately synchronised calls, each with tables of its own
    want = []
    for lo, hi in sets:
        c = Call(lo, hi)
        c.enqueue(*tables(lo, hi))
        assert L.torj_trace_check(hplasma.handle, stream.cuda_stream) == 0
        want.append(c.out())
    # back to back: one set of table arrays, overwritten between the calls
    off, om, md = (np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(8, dtype=np.int32))
    calls = []
    for lo, hi in sets:
        o, w_, m_ = tables(lo, hi)
        off[:], om[:], md[:] = 0, 0.0, 0
        off[:len(o)], om[:len(w_)], md[:len(m_)] = o, w_, m_
        calls.append(Call(lo, hi))
        calls[-1].enqueue(off, om, md)
    assert L.torj_trace_check(hplasma.handle, stream.cuda_stream) == 0
    for c, ref in zip(calls, want):
        for a, r in zip(c.out(), ref):
            assert np.array_equal(a, r)
    # the counters: the sums of the beams' own launches'
    tot = np.zeros(8, dtype=np.int64)
    for k in range(6):
        sl = slice(b["off"][k], b["off"][k + 1])
        n = sl.stop - sl.start
        if n == 0:
            continue
        c1 = T._lib.TraceCfg(b["omega"][k], b["mode"][k], DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, 0)
        x0, N0 = t(b["xp"][sl].T), t(b["Np"][sl].T)
        state = torch.empty((7, n), dtype=torch.float64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        steps = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.zeros(8, dtype=torch.int64, device=dev)
        T._lib.check(L.torj_trace_device_ex(hplasma.handle, c1, n, x0.data_ptr(), N0.data_ptr(), None, 0, None,
                                            None, None, state.data_ptr(), status.data_ptr(), steps.data_ptr(),
                                            None, None, None, cnt.data_ptr(), stream.cuda_stream))
        assert L.torj_trace_check(hplasma.handle, stream.cuda_stream) == 0
        tot += cnt.cpu().numpy()
    got = want[0][3] + want[1][3]
    assert np.array_equal(got, tot), (got, tot)
    assert tot[0] == sum(int(r[2].sum()) for r in want) and tot[1] == 4 * tot[0]
    # a grid that does not increase: found by the launch, reported by the check
    bad = GRID.copy()
    bad[50] = bad[49]
    c = Call(1, 4, grid=bad)
    c.enqueue(*tables(1, 4))
    assert L.torj_trace_check(hplasma.handle, stream.cuda_stream) != 0
    assert b"strictly increasing" in L.torj_last_error()
    c = Call(1, 4, grid=GRID)
    c.enqueue(*tables(1, 4))
    assert L.torj_trace_check(hplasma.handle, stream.cuda_stream) == 0


def test_beams_workspace_beyond_budget_is_an_error(gpu, T, hplasma, beams, monkeypatch):
    """The reference deposition's workspace holds all rays of the launch; beyond the
    budget the call fails, naming the budget and the way out (no ray batches here)."""
    b = beams
    monkeypatch.setenv("TORJ_WS_GB", "0.001")  # 1 MiB; the 111 rays need ~60 MB
    with pytest.raises(T.TorjError, match=r"exceeds the budget of \d+ bytes \(TORJ_WS_GB\).*separate calls"):
        T.trace_beams(hplasma, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], **KW, **depo_kw(b, "reference"))
    monkeypatch.delenv("TORJ_WS_GB")
    m = T.trace_beams(hplasma, b["off"][:3], b["omega"][:2], b["mode"][:2], b["xp"][:51], b["Np"][:51],
                      ds=DS, n_steps=200, **depo_kw(b, "reference", slice(0, 51)))
    assert (m.steps == 200).all()


def test_ray_entry_beams_equals_per_beam(gpu, T, hplasma, beams):
    """ray_entry_beams against ray_entry(gpu=True) per beam: the six beams' full fans
    and a seventh whose third ray points away from the plasma (not OK)."""
    pos, dirs, off, omega, mode = [], [], [0], [], []
    for f, m, pol, tor, k in BEAMS:
        p, d, _ = fan(T, f, pol, tor)
        pos.append(p[:k]), dirs.append(d[:k])
        off.append(off[-1] + k), omega.append(2 * np.pi * f), mode.append(m)
    p, d, _ = fan(T, 92.5e9, 30.0, 0.0)
    d = d[:6].copy()
    d[2] = -d[2]
    pos.append(p[:6]), dirs.append(d)
    off.append(off[-1] + 6), omega.append(2 * np.pi * 92.5e9), mode.append(1)
    got = T.ray_entry_beams(hplasma, off, omega, mode, np.concatenate(pos), np.concatenate(dirs))
    bad = False
    for k in range(len(omega)):
        if off[k] == off[k + 1]:
            continue
        want = T.ray_entry(hplasma, pos[k], dirs[k], omega[k], mode[k], gpu=True)
        for a, r in zip(got, want):
            assert np.array_equal(a[off[k]:off[k + 1]], r, equal_nan=True)
        bad |= bool((want[3] != T.OK).any())
    assert bad
    assert (got[3][:off[-2]] == T.OK).all() and got[3][off[-2] + 2] != T.OK


def test_make_beams_equals_make_beam(gpu, T, hplasma):
    """make_beams on three launchers against make_beam on each (s_max = 0.2: 2 000
    steps, the reference deposition, 16 lanes per ray in both)."""
    from torj_hip import synthetic as S

    s = S.SETUP
    base = (s["R0"], s["phi0"], s["z0"])
    rest = (s["spot_size"], s["inverse_curvature_radius"])
    launchers = [(*base, 0.0, np.deg2rad(30.0), *rest, 92.5e9, 1),
                 (*base, np.deg2rad(-5.0), np.deg2rad(35.0), *rest, 100e9, 1),
                 (*base, np.deg2rad(5.0), np.deg2rad(25.0), *rest, 85.5e9, -1)]
    got = T.make_beams(hplasma, launchers, 0.2, GRID)
    assert len(got) == 3
    for la, g in zip(launchers, got):
        want = T.make_beam(hplasma, *la, 0.2, GRID)
        assert len(g) == len(want) == 6
        for k in range(3):  # arc lengths, trajectories, ray powers: a list per ray
            assert len(g[k]) == len(want[k]) == 46
            for a, r in zip(g[k], want[k]):
                assert np.array_equal(a, r)
        assert np.array_equal(g[3], want[3])
        assert g[4] == want[4]
        assert np.array_equal(g[5], want[5])
    with pytest.raises(T.RayEntryError, match="beam 1"):
        bad = list(launchers)
        bad[1] = (*base, 0.0, np.deg2rad(210.0), *rest, 92.5e9, 1)  # launched away from the plasma
        T.make_beams(hplasma, bad, 0.2, GRID)
