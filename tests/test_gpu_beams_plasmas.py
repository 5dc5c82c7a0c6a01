"""Many small beams through differing plasmas in one launch
(torj_trace_beams_plasmas[_device], torj_ray_entry_beams_plasmas_gpu, make_beams
with plasmas=) on the GPU: bit-identical to one launch per beam on that beam's own
plasma with the same lanes per ray, and each beam against the CPU oracle of its
plasma with its own frequency and mode.

Workload: tests/test_gpu_beams.py's -- SETUP's launch point, the default 46-ray
fan, 12 000 steps of 1e-4 m with termination checks every 120, 200 shell
boundaries, trajectory samples every 1 000 steps -- through four synthetic
tokamaks: P0 the default, P1 hotter and thinner, P2 colder on another grid
(72 x 64 nodes, other ranges), P3 denser.  Seven beams, 124 rays: 46 + 46 + 5 + 0
+ 1 + 13 + 13, so that beams end inside a wave at both 4 and 64 rays per wave, one
is empty and one is a single ray, with the plasma indices interleaved.  Beams 0
and 1 are the same launcher through P0 and P1: in the oracle, beam 1's rays traced
through P0 instead differ by up to 5.9 in tau and 7 680 steps, so a launch that
ignores beam_plasma cannot pass.

P1, P2 and P3 are handles no test uses before a multi-plasma call does: their
device state is created by that call (the coefficients of a handle are uploaded on
its first GPU use)."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import _compare_trace

pytestmark = pytest.mark.gpu

DS, N_STEPS, CHUNK, STRIDE = 1e-4, 12000, 120, 1000
GRID = np.linspace(0.0, 1.0, 200)
PLASMAS = (
    dict(),
    dict(Te0=6000, ne_scale=0.6),
    dict(nR=72, nZ=64, R_range=(0.9, 2.7), Z_range=(-0.9, 0.9), Te0=1500),
    dict(ne_scale=1.5),
)
# frequency, mode, steering pol / tor (degrees), rays taken from the 46-ray fan, plasma
BEAMS = (
    (92.5e9, 1, 30.0, 0.0, 46, 0),
    (92.5e9, 1, 30.0, 0.0, 46, 1),
    (92.5e9, -1, 30.0, 0.0, 5, 2),
    (140e9, 1, 30.0, 0.0, 0, 1),
    (110e9, 1, 30.0, 0.0, 1, 2),
    (100e9, 1, 35.0, -5.0, 13, 3),
    (85.5e9, -1, 25.0, 5.0, 13, 0),
)
NB = len(BEAMS)
BP = [b[5] for b in BEAMS]


def fan(T, f, pol, tor):
    from torj_hip import synthetic as S

    s = S.SETUP
    N0 = T.pol_tor_angles_2_vector(np.deg2rad(pol), np.deg2rad(tor))
    return T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"],
                                    s["inverse_curvature_radius"], f)


@pytest.fixture(scope="module")
def eqs():
    from torj_hip import synthetic as S

    return [S.circular_tokamak(**kw) for kw in PLASMAS]


@pytest.fixture(scope="module")
def pl(T, eqs):
    """The four plasmas' handles, fresh, and a fifth that only launches (its own plasma,
    unlike any of the four, is never a beam's)."""
    from torj_hip import synthetic as S

    hs = [T.Plasma(*S.plasma_args(eq)) for eq in eqs]
    other = T.Plasma(*S.plasma_args(S.circular_tokamak(Te0=2000, ne_scale=0.8)))
    return hs, other


@pytest.fixture(scope="module")
def beams(T, pl):
    """The seven beams' concatenated launch and entry states (each beam entered into its
    own plasma, on the host: no GPU use of the handles) and their tables."""
    hs, _ = pl
    pos, dirs, w, xp, Np, s0, off, omega, mode = [], [], [], [], [], [], [0], [], []
    for f, m, pol, tor, k, j in BEAMS:
        p, d, ww = fan(T, f, pol, tor)
        assert len(ww) == 46
        om = 2 * np.pi * f
        x, N, s, st = T.ray_entry(hs[j], p, d, om, m)
        assert (st == 0).all()
        for lst, a in ((pos, p), (dirs, d), (w, ww), (xp, x), (Np, N), (s0, s)):
            lst.append(a[:k])
        off.append(off[-1] + k)
        omega.append(om)
        mode.append(m)
    cat = {k: np.concatenate(v) for k, v in dict(pos=pos, dirs=dirs, w=w, xp=xp, Np=Np, s0=s0).items()}
    assert off == [0, 46, 92, 97, 97, 98, 111, 124]
    return dict(off=off, omega=omega, mode=mode, **cat)


KW = dict(ds=DS, n_steps=N_STEPS, chunk_steps=CHUNK, traj_stride=STRIDE)


def depo_kw(b, deposition, sl=slice(None)):
    if deposition == "none":
        return {}
    kw = dict(psi_grid=GRID, weights=b["w"][sl], deposition=deposition)
    if deposition == "reference":
        kw.update(x_launch=b["pos"][sl], s0=b["s0"][sl])
    return kw


def multi(T, p, hs, b, deposition, kw=KW):
    return T.trace_beams(p, b["off"], b["omega"], b["mode"], b["xp"], b["Np"], **kw, **depo_kw(b, deposition),
                         plasmas=hs, beam_plasma=BP)


def single(T, hs, b, k, deposition, kw=KW):
    """beam k alone through its own plasma: one T.trace"""
    sl = slice(b["off"][k], b["off"][k + 1])
    return sl, T.trace(hs[BP[k]], b["xp"][sl], b["Np"][sl], b["omega"][k], b["mode"][k], **kw,
                       **depo_kw(b, deposition, sl))


def per_ray_equal(m, sl, s):
    assert np.array_equal(m.state[sl], s.state)
    assert np.array_equal(m.status[sl], s.status)
    assert np.array_equal(m.steps[sl], s.steps)
    assert np.array_equal(m.P_dep[sl], s.P_dep)
    if s.traj is not None:
        assert np.array_equal(m.traj[sl], s.traj, equal_nan=True)


def sched_all(handles, mode):
    for h in handles:
        h.set_sched(mode)


def test_first_gpu_use_of_listed_handles(gpu, T, eqs, beams):
    """Handles whose first GPU use is the multi-plasma call, the launching one included:
    the call creates their device state before it reads their coefficients.  (200 steps;
    the module's handles serve the other tests.)"""
    from torj_hip import synthetic as S

    b = beams
    hs = [T.Plasma(*S.plasma_args(eq)) for eq in eqs]
    kw = dict(ds=DS, n_steps=200, chunk_steps=20)
    m = multi(T, T.Plasma(*S.plasma_args(eqs[3])), hs, b, "reference", kw)
    assert (m.steps > 0).all()
    for k in (0, 1, 4):
        sl, s = single(T, hs, b, k, "reference", kw)
        per_ray_equal(m, sl, s)
        assert np.array_equal(m.dP_shell[k], s.dP_shell)


@pytest.mark.parametrize("launcher", ["listed", "unlisted"])
@pytest.mark.parametrize("deposition", ["none", "reference"])
@pytest.mark.parametrize("lanes", [16, 1])
def test_beams_plasmas_equal_single_launches(gpu, T, pl, beams, lanes, deposition, launcher):
    """One launch through four plasmas against one launch per beam on that beam's plasma
    with the same lanes per ray: every per-ray output and, with the reference deposition,
    every dP_shell row is the same bits.  Launched by P0 (listed) and by a fifth handle."""
    hs, other = pl
    p = hs[0] if launcher == "listed" else other
    b = beams
    every = hs + [other]
    try:
        sched_all(every, 2 if lanes == 16 else 0)
        m = multi(T, p, hs, b, deposition)
        assert m.dP_shell.shape == (NB, len(GRID) + 1 if deposition != "none" else 1)
        for k in range(NB):
            if b["off"][k] == b["off"][k + 1]:
                assert not m.dP_shell[k].any()  # the empty beam's row
                continue
            sl, s = single(T, hs, b, k, deposition)
            per_ray_equal(m, sl, s)
            if deposition == "reference":
                assert np.array_equal(m.dP_shell[k], s.dP_shell)
        if deposition == "reference":
            assert m.dP_shell[:, :-2].any()
        # beams 0 and 1, one launcher through P0 and P1, do differ
        assert not np.array_equal(m.steps[0:46], m.steps[46:92])
    finally:
        sched_all(every, -1)


def test_beams_plasmas_binned_equal_single_launches(gpu, T, pl, beams):
    """Binned deposition (one lane per ray): per-ray outputs the same bits, the shells'
    atomic sums to their order -- the bar of test_beams_binned_equal_single_launches."""
    hs, _ = pl
    b = beams
    try:
        sched_all(hs, 0)
        m = multi(T, hs[0], hs, b, "binned")
        for k in range(NB):
            if b["off"][k] == b["off"][k + 1]:
                assert not m.dP_shell[k].any()
                continue
            sl, s = single(T, hs, b, k, "binned")
            per_ray_equal(m, sl, s)
            err = np.abs(m.dP_shell[k] - s.dP_shell).max()
            print(f"beam {k}: dP row differs by {err:.3e} of max {np.abs(s.dP_shell).max():.3e}")
            assert err <= 1e-12 * np.abs(s.dP_shell).max()
    finally:
        sched_all(hs, -1)


class _Beam:
    """rays sl of a multi-beam TraceResult as _compare_trace reads them"""

    def __init__(self, m, sl):
        self.state, self.status, self.steps = m.state[sl], m.status[sl], m.steps[sl]


def test_beams_plasmas_match_oracle(gpu, T, O, pl, eqs, beams):
    """The automatic path with binned deposition, each beam against the oracle of ITS
    plasma with its own frequency and mode, at test_beams_match_oracle's bars.  (A launch
    with one plasma for all beams cannot pass this.)"""
    from torj_hip import synthetic as S

    hs, _ = pl
    b = beams
    oracles = [O.OraclePlasma(*S.plasma_args(eq)) for eq in eqs]
    m = multi(T, hs[0], hs, b, "binned")
    seen = set()
    for k in range(NB):
        sl = slice(b["off"][k], b["off"][k + 1])
        if sl.start == sl.stop:
            continue
        o = oracles[BP[k]].trace(b["xp"][sl], b["Np"][sl], b["omega"][k], b["mode"][k], DS, N_STEPS,
                                 chunk_steps=CHUNK, psi_grid=GRID, weights=b["w"][sl])
        seen |= set(o["status"].tolist())
        _compare_trace(_Beam(m, sl), o)
        scale = max(np.abs(o["dP"]).max(), 1e-300)
        err = np.abs(m.dP_shell[k, :-1] - o["dP"]).max()
        print(f"beam {k}: dP differs from the oracle's by {err:.3e} of max {scale:.3e}")
        assert err <= 1e-10 * scale
        assert np.abs(m.P_dep[sl] - o["Pdep"]).max() <= 1e-10 * max(o["Pdep"].max(), 1e-300)
    # all three ends occur in the oracle's own results (else the workload is too short)
    assert {T.OK, T.LEFT_PLASMA, T.ABSORBED} <= seen


def test_beams_plasmas_device_back_to_back(gpu, T, pl, beams):
    """Two torj_trace_beams_plasmas_device calls on one stream with no sync between them,
    the five host tables overwritten with the second call's values as soon as the first has
    returned, then one torj_trace_check on the launching handle: each call saw its own
    tables.  The counters are the sums of the beams' own launches'."""
    import torch

    hs, other = pl
    b = beams
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    L = T.lib()
    cfg = T._lib.TraceCfg(0.0, 0, DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, 0)
    # beams 0..3 (97 rays) through [P0, P1, P2]; beams 4..6 (27 rays) through [P3, P0, P2]
    sets = ((0, 4, (0, 1, 2), (0, 1, 2, 1)), (4, 7, (3, 0, 2), (2, 0, 1)))
    for lo, hi, listed, idx in sets:
        assert [listed[i] for i in idx] == BP[lo:hi]

    def t(a, dtype=torch.float64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dtype)

    def tables(lo, hi, listed, idx):
        off = np.array(b["off"][lo:hi + 1], dtype=np.int32) - b["off"][lo]
        return (off, np.array(b["omega"][lo:hi]), np.array(b["mode"][lo:hi], dtype=np.int32),
                [hs[j].handle.value for j in listed], np.array(idx, dtype=np.int32))

    class Call:
        def __init__(self, lo, hi):
            sl = slice(b["off"][lo], b["off"][hi])
            self.n, self.nb = sl.stop - sl.start, hi - lo
            self.x0, self.N0 = t(b["xp"][sl].T), t(b["Np"][sl].T)
            self.state = torch.empty((7, self.n), dtype=torch.float64, device=dev)
            self.status = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.steps = torch.empty(self.n, dtype=torch.int32, device=dev)
            self.counters = torch.zeros(8, dtype=torch.int64, device=dev)

        def enqueue(self, off, om, md, handles, n_pl, bpl):
            T._lib.check(L.torj_trace_beams_plasmas_device(
                other.handle, n_pl, handles, T._lib.iptr(bpl), cfg, self.nb, T._lib.iptr(off), T._lib.dptr(om),
                T._lib.iptr(md), self.x0.data_ptr(), self.N0.data_ptr(), None, 0, None, None, None,
                self.state.data_ptr(), self.status.data_ptr(), self.steps.data_ptr(), None, None, None,
                self.counters.data_ptr(), stream.cuda_stream))

        def out(self):
            return [a.cpu().numpy() for a in (self.state, self.status, self.steps, self.counters)]

    # separately synchronised calls, each with tables of its own
    want = []
    for lo, hi, listed, idx in sets:
        off, om, md, hv, bpl = tables(lo, hi, listed, idx)
        c = Call(lo, hi)
        c.enqueue(off, om, md, (ctypes.c_void_p * len(hv))(*hv), len(hv), bpl)
        assert L.torj_trace_check(other.handle, stream.cuda_stream) == 0
        want.append(c.out())
    # back to back: one set of table arrays, overwritten between the calls
    off, om, md, bpl = (np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros(8, dtype=np.int32),
                        np.zeros(8, dtype=np.int32))
    handles = (ctypes.c_void_p * 4)()
    calls = []
    for lo, hi, listed, idx in sets:
        o, w_, m_, hv, i_ = tables(lo, hi, listed, idx)
        off[:], om[:], md[:], bpl[:] = 0, 0.0, 0, 0
        off[:len(o)], om[:len(w_)], md[:len(m_)], bpl[:len(i_)] = o, w_, m_, i_
        for j in range(4):
            handles[j] = hv[j] if j < len(hv) else None
        calls.append(Call(lo, hi))
        calls[-1].enqueue(off, om, md, handles, len(hv), bpl)
    assert L.torj_trace_check(other.handle, stream.cuda_stream) == 0
    for c, ref in zip(calls, want):
        for a, r in zip(c.out(), ref):
            assert np.array_equal(a, r)
    # the counters: the sums of the beams' own launches', each on its own plasma
    tot = np.zeros(8, dtype=np.int64)
    for k in range(NB):
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
        h = hs[BP[k]].handle
        T._lib.check(L.torj_trace_device_ex(h, c1, n, x0.data_ptr(), N0.data_ptr(), None, 0, None, None, None,
                                            state.data_ptr(), status.data_ptr(), steps.data_ptr(), None, None,
                                            None, cnt.data_ptr(), stream.cuda_stream))
        assert L.torj_trace_check(h, stream.cuda_stream) == 0
        tot += cnt.cpu().numpy()
    got = want[0][3] + want[1][3]
    assert np.array_equal(got, tot), (got, tot)
    assert tot[0] == sum(int(r[2].sum()) for r in want) and tot[1] == 4 * tot[0]


def test_null_stream_equals_explicit_stream(gpu, T, pl, beams):
    """The three device-pointer traces with stream = 0 against the same call on a stream
    of the caller's: the NULL stream's fork onto the handle's stream and the join back.
    Beams 2, 3 and 4 of the fixture (5, 0 and 1 rays) through [P2, P1]; 1 200 steps, the
    reference deposition on 20 boundaries, trajectory samples every 600 steps.  After the
    stream-0 call the outputs are read by plain default-stream copies, with no
    synchronize on the handle's stream: only the join orders them after the trace."""
    import torch

    hs, _ = pl
    b = beams
    dev = torch.device("cuda", 0)
    L = T.lib()
    lo, hi = 2, 5
    sl = slice(b["off"][lo], b["off"][hi])
    n, nb, n5 = sl.stop - sl.start, hi - lo, b["off"][lo + 1] - b["off"][lo]
    assert (n, n5, BP[lo:hi]) == (6, 5, [2, 1, 2])
    off = np.array(b["off"][lo:hi + 1], dtype=np.int32) - b["off"][lo]
    om, md = np.array(b["omega"][lo:hi]), np.array(b["mode"][lo:hi], dtype=np.int32)
    handles = (ctypes.c_void_p * 2)(hs[2].handle.value, hs[1].handle.value)
    bpl = np.array([0, 1, 0], dtype=np.int32)
    grid = np.linspace(0.0, 1.0, 20)
    n_steps, stride = 1200, 600
    n_save = n_steps // stride

    def t(a, dtype=torch.float64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dtype)

    x0, N0, w = t(b["xp"][sl].T), t(b["Np"][sl].T), t(b["w"][sl])
    xl, s0, g = t(b["pos"][sl].T), t(b["s0"][sl]), t(grid)
    x5, N5, xl5 = t(b["xp"][sl][:n5].T), t(b["Np"][sl][:n5].T), t(b["pos"][sl][:n5].T)

    def run(which, stream):
        """one call on `stream` (0: the NULL stream); the outputs, read on torch's current stream"""
        m, rows = (n5, 1) if which == "single" else (n, nb)
        state = torch.zeros((7, m), dtype=torch.float64, device=dev)
        status = torch.zeros(m, dtype=torch.int32, device=dev)
        steps = torch.zeros(m, dtype=torch.int32, device=dev)
        dP = torch.zeros((rows, len(grid) + 1), dtype=torch.float64, device=dev)
        Pdep = torch.zeros(m, dtype=torch.float64, device=dev)
        traj = torch.zeros((n_save, 5, m), dtype=torch.float64, device=dev)
        out = (state, status, steps, dP, Pdep, traj)
        tail = [len(grid), g.data_ptr()]
        if which == "single":
            cfg = T._lib.TraceCfg(om[0], int(md[0]), DS, n_steps, CHUNK, 1.0, 1e-6, 1, stride, 1)
            tail += [xl5.data_ptr(), s0.data_ptr()] + [a.data_ptr() for a in out] + [None, stream]
            rc = L.torj_trace_device_ex(hs[2].handle, cfg, n5, x5.data_ptr(), N5.data_ptr(), w.data_ptr(), *tail)
        else:
            cfg = T._lib.TraceCfg(0.0, 0, DS, n_steps, CHUNK, 1.0, 1e-6, 1, stride, 1)
            tabs = (cfg, nb, T._lib.iptr(off), T._lib.dptr(om), T._lib.iptr(md), x0.data_ptr(), N0.data_ptr(),
                    w.data_ptr())
            tail += [xl.data_ptr(), s0.data_ptr()] + [a.data_ptr() for a in out] + [None, stream]
            if which == "beams":
                rc = L.torj_trace_beams_device(hs[2].handle, *tabs, *tail)
            else:
                rc = L.torj_trace_beams_plasmas_device(hs[2].handle, 2, handles, T._lib.iptr(bpl), *tabs, *tail)
        T._lib.check(rc)
        got = [a.cpu().numpy() for a in out]
        assert L.torj_trace_check(hs[2].handle, stream) == 0
        return got

    side = torch.cuda.Stream(dev)
    assert side.cuda_stream != 0
    for which in ("single", "beams", "plasmas"):
        null = run(which, 0)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            assert torch.cuda.current_stream(dev).cuda_stream == side.cuda_stream
            own = run(which, side.cuda_stream)
        side.synchronize()
        for a, r in zip(null, own):
            assert np.array_equal(a, r, equal_nan=a.dtype.kind == "f")
        assert (null[2] > 0).all(), which  # every ray stepped


def test_ray_entry_beams_plasmas_equals_per_beam(gpu, T, pl):
    """ray_entry_beams(plasmas=) against ray_entry(gpu=True) on each beam's plasma: the
    seven beams' fans and an eighth whose third ray points away from the plasma (not OK)."""
    hs, other = pl
    pos, dirs, off, omega, mode = [], [], [0], [], []
    for f, m, pol, tor, k, _ in BEAMS:
        p, d, _w = fan(T, f, pol, tor)
        pos.append(p[:k]), dirs.append(d[:k])
        off.append(off[-1] + k), omega.append(2 * np.pi * f), mode.append(m)
    p, d, _w = fan(T, 92.5e9, 30.0, 0.0)
    d = d[:6].copy()
    d[2] = -d[2]
    pos.append(p[:6]), dirs.append(d)
    off.append(off[-1] + 6), omega.append(2 * np.pi * 92.5e9), mode.append(1)
    bp = BP + [3]
    got = T.ray_entry_beams(other, off, omega, mode, np.concatenate(pos), np.concatenate(dirs), plasmas=hs,
                            beam_plasma=bp)
    bad = False
    for k in range(len(omega)):
        if off[k] == off[k + 1]:
            continue
        want = T.ray_entry(hs[bp[k]], pos[k], dirs[k], omega[k], mode[k], gpu=True)
        for a, r in zip(got, want):
            assert np.array_equal(a[off[k]:off[k + 1]], r, equal_nan=True)
        bad |= bool((want[3] != T.OK).any())
    assert bad
    assert (got[3][:off[-2]] == T.OK).all() and got[3][off[-2] + 2] != T.OK
    # the same launcher is refracted differently into P0 and P1 (beams 0 and 1): N_plasma
    assert not np.array_equal(got[1][0:46], got[1][46:92])


def test_make_beams_plasmas_equals_make_beam(gpu, T, pl):
    """make_beams on three launchers over P0 / P1 / P3 against make_beam on each plasma
    (s_max = 0.2: 2 000 steps, the reference deposition), dP_dV with that plasma's shell
    volumes included."""
    from torj_hip import synthetic as S

    hs, _ = pl
    s = S.SETUP
    base = (s["R0"], s["phi0"], s["z0"])
    rest = (s["spot_size"], s["inverse_curvature_radius"])
    launchers = [(*base, 0.0, np.deg2rad(30.0), *rest, 92.5e9, 1),
                 (*base, np.deg2rad(-5.0), np.deg2rad(35.0), *rest, 100e9, 1),
                 (*base, np.deg2rad(5.0), np.deg2rad(25.0), *rest, 85.5e9, -1)]
    listed, bp = [hs[0], hs[1], hs[3]], [0, 1, 2]
    got = T.make_beams(hs[0], launchers, 0.2, GRID, plasmas=listed, beam_plasma=bp)
    assert len(got) == 3
    for la, g, q in zip(launchers, got, listed):
        want = T.make_beam(q, *la, 0.2, GRID)
        assert len(g) == len(want) == 6
        for k in range(3):  # arc lengths, trajectories, ray powers: a list per ray
            assert len(g[k]) == len(want[k]) == 46
            for a, r in zip(g[k], want[k]):
                assert np.array_equal(a, r)
        assert np.array_equal(g[3], want[3])
        assert g[4] == want[4]
        assert np.array_equal(g[5], want[5])


def test_one_plasma_is_trace_beams(gpu, T, pl, beams):
    """n_plasmas = 1 and every beam_plasma 0: the outputs of torj_trace_beams on that
    plasma with the same tables, bit for bit (reference deposition, automatic lanes)."""
    hs, other = pl
    b = beams
    args = (b["off"], b["omega"], b["mode"], b["xp"], b["Np"])
    want = T.trace_beams(hs[0], *args, **KW, **depo_kw(b, "reference"))
    for p in (hs[0], other):
        got = T.trace_beams(p, *args, **KW, **depo_kw(b, "reference"), plasmas=[hs[0]], beam_plasma=[0] * NB)
        per_ray_equal(got, slice(None), want)
        assert np.array_equal(got.dP_shell, want.dP_shell)
