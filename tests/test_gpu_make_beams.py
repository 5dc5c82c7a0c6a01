"""torj_make_beams on the GPU (make_beams_c in the mirror): make_beams as one C call that
reports, per beam, which part of the fan entered the plasma, and traces the rest.

Workload: SETUP's launch point, the default 46-ray fans, s_max = 0.2 (2 000 steps of
1e-4 m), the reference deposition on 200 shell boundaries, a trajectory sample per step.
Where every ray enters, the call is make_beams bit for bit.  A launcher whose fan grazes
the plasma (GRAZING: 32 of 46 rays enter) and one that misses it (MISSING) are
preconditions checked on the CPU in tests/test_make_beams_capi.py.

Every test here fails on a library without the symbol torj_make_beams."""
import numpy as np
import pytest

from test_make_beams_capi import (GRAZING_FIRST_BAD, GRAZING_OK, GRAZING_POL, GRID, MISSING_POL, host_entry,
                                  launcher)

pytestmark = pytest.mark.gpu

S_MAX, N_STEPS = 0.2, 2000
# the three launchers of test_make_beams_plasmas_equals_make_beam (tests/test_gpu_beams_plasmas.py)
LAUNCHERS = [launcher(30.0, 0.0, 92.5e9, 1), launcher(35.0, -5.0, 100e9, 1), launcher(25.0, 5.0, 85.5e9, -1)]
GRAZING, MISSING = launcher(GRAZING_POL), launcher(MISSING_POL)
PLASMAS = (dict(), dict(Te0=6000, ne_scale=0.6), dict(ne_scale=1.5))


def new_plasma(T, **kw):
    from torj_hip import synthetic as S

    return T.Plasma(*S.plasma_args(S.circular_tokamak(**kw)))


@pytest.fixture(scope="module")
def hs(T):
    return [new_plasma(T, **kw) for kw in PLASMAS]


def seq_sum(v):
    """the sum in index order from 0.0, one rounding per addition (torj_beam_result's w_ok)"""
    acc = 0.0
    for x in v:
        acc += float(x)
    return acc


def tuples_equal(g, want, n_rays):
    assert len(g) == len(want) == 6
    for k in range(3):  # arc lengths, trajectories, ray powers: a list per ray
        assert len(g[k]) == len(want[k]) == n_rays
        for a, r in zip(g[k], want[k]):
            assert np.array_equal(a, r)
    assert np.array_equal(g[3], want[3])
    assert g[4] == want[4]
    assert np.array_equal(g[5], want[5])


@pytest.mark.parametrize("sched", [0, 2])
def test_everything_equals_make_beams(gpu, T, hs, sched):
    """one plasma, then three listed ones: every element of every tuple is make_beams',
    with 1 and with 16 lanes per ray"""
    try:
        hs[0].set_sched(sched)  # the launching handle's knob
        for sel in (dict(), dict(plasmas=hs, beam_plasma=[0, 1, 2])):
            got, results = T.make_beams_c(hs[0], LAUNCHERS, S_MAX, GRID, **sel)
            want = T.make_beams(hs[0], LAUNCHERS, S_MAX, GRID, **sel)
            assert len(got) == len(results) == len(want) == 3
            for g, r, w in zip(got, results, want):
                tuples_equal(g, w, 46)
                assert (r["n_rays"], r["n_ok"], r["first_bad_ray"], r["first_bad_status"]) == (46, 46, -1, 0)
                assert r["w_ok"] == seq_sum(w[5])
                assert r["deposited_power"] == w[4]
    finally:
        hs[0].set_sched(-1)


def test_failures_are_reported_not_fatal(gpu, T, hs):
    """[good, grazing, missing, good]: the call succeeds, the good beams are make_beam's, the
    grazing beam is torj_trace_beams on exactly its entered rays with their launched weights,
    the missing beam is an empty row, and the failed rays carry their entry status"""
    P = hs[0]
    las = [LAUNCHERS[0], GRAZING, MISSING, LAUNCHERS[1]]
    try:
        P.set_sched(0)  # one lane per ray on every side: the kept counts never change the lanes
        m = T.solve.make_beams_arrays(P, las, S_MAX, GRID)  # raises unless the call returned 0
        got, results = T.make_beams_c(P, las, S_MAX, GRID)
        good = [T.make_beam(P, *las[b], S_MAX, GRID) for b in (0, 3)]
        # the grazing launcher's own fan and GPU entry, and the trace of what entered
        pos, dirs, w, _, _, _, st_host = host_entry(T, P, GRAZING)
        om = 2.0 * np.pi * GRAZING[7]
        xp, Np, s0, st = T.ray_entry(P, pos, dirs, om, 1, gpu=True)
        ok = np.flatnonzero(st == 0)
        ref = T.trace_beams(P, [0, len(ok)], [om], [1], xp[ok], Np[ok], ds=1e-4, n_steps=N_STEPS, psi_grid=GRID,
                            weights=w[ok], traj_stride=1, deposition="reference", x_launch=pos[ok], s0=s0[ok])
    finally:
        P.set_sched(-1)
    off, res = m["off"], m["res"]
    assert list(off) == [0, 46, 92, 138, 184]
    assert [r["n_rays"] for r in results] == [46] * 4
    assert results == m["results"]
    # good beams
    for b, want in zip((0, 3), good):
        tuples_equal(got[b], want, 46)
        assert (results[b]["n_ok"], results[b]["first_bad_ray"], results[b]["first_bad_status"]) == (46, -1, 0)
        assert results[b]["deposited_power"] == want[4]
    # the grazing beam: tallies as the host entry gives them
    r = results[1]
    assert np.array_equal(st, st_host)
    bad = np.flatnonzero(st_host != 0)
    assert r["n_ok"] == int((st_host == 0).sum()) == GRAZING_OK
    assert (r["first_bad_ray"], r["first_bad_status"]) == (int(bad[0]), int(st_host[bad[0]])) == GRAZING_FIRST_BAD
    assert r["w_ok"] == seq_sum(w[ok]) and 0.0 < r["w_ok"] < 1.0
    sl = slice(off[1], off[2])
    assert np.array_equal(m["pos"][sl], pos) and np.array_equal(m["dirs"][sl], dirs) and np.array_equal(m["w"][sl], w)
    assert np.array_equal(m["entry_status"][sl], st)
    g = off[1] + ok  # launched indices of its entered rays
    for a, b in ((m["xp"][g], xp[ok]), (m["Np"][g], Np[ok]), (m["s0"][g], s0[ok]), (res.state[g], ref.state),
                 (res.status[g], ref.status), (res.steps[g], ref.steps), (res.P_dep[g], ref.P_dep)):
        assert np.array_equal(a, b)
    assert np.array_equal(res.traj[g], ref.traj, equal_nan=True)
    assert (ref.steps > 0).all()
    row = np.zeros(len(GRID))
    row[:-1] = ref.dP_shell[0, :len(GRID) - 1] / P.shell_volumes(GRID)
    assert np.array_equal(m["dP_dV"][1], row)
    assert r["deposited_power"] == ref.dP_shell[0, len(GRID)]
    assert len(got[1][0]) == len(got[1][1]) == len(got[1][2]) == GRAZING_OK
    assert np.array_equal(got[1][5], w[ok]) and np.array_equal(got[1][3], row)
    # the missing beam: an empty row
    r = results[2]
    assert (r["n_ok"], r["first_bad_ray"], r["first_bad_status"]) == (0, 0, 5)
    assert r["w_ok"] == 0.0 and r["deposited_power"] == 0.0
    assert not m["dP_dV"][2].any()
    assert [len(x) for x in got[2][:3]] == [0, 0, 0] and len(got[2][5]) == 0
    # every failed ray: its entry status, no steps, no power, NaN state and samples
    failed = np.flatnonzero(m["entry_status"] != 0)
    assert len(failed) == (46 - GRAZING_OK) + 46
    assert set(m["entry_status"][failed]) <= {4, 5}
    assert np.array_equal(res.status[failed], m["entry_status"][failed])
    assert not res.steps[failed].any() and not res.P_dep[failed].any()
    assert np.isnan(res.state[failed]).all() and np.isnan(res.traj[failed]).all()
    entered = np.flatnonzero(m["entry_status"] == 0)
    assert not np.isnan(res.state[entered]).any() and (res.steps[entered] > 0).all()


def test_absorbing_beams(gpu, T, hs):
    """Beyond the 0.2 m of the tests above, where no ray has reached the resonance yet and
    every dP_dV row is 0: test_gpu_beams.py's 12 000 steps (a sample per 1 000), so that the
    rows, the division by the shell volumes and deposited_power carry power.  [good, grazing,
    missing] with one lane per ray: the good beam is make_beam's, the grazing beam
    torj_trace_beams' on its entered rays with their launched weights."""
    P, s_max, stride = hs[0], 1.2, 1000
    las = [LAUNCHERS[0], GRAZING, MISSING]
    try:
        P.set_sched(0)
        m = T.solve.make_beams_arrays(P, las, s_max, GRID, traj_stride=stride)
        got, results = T.make_beams_c(P, las, s_max, GRID, traj_stride=stride)
        want = T.make_beam(P, *las[0], s_max, GRID, traj_stride=stride)
        pos, dirs, w = m["pos"][46:92], m["dirs"][46:92], m["w"][46:92]
        om = 2.0 * np.pi * GRAZING[7]
        xp, Np, s0, st = T.ray_entry(P, pos, dirs, om, 1, gpu=True)
        ok = np.flatnonzero(st == 0)
        ref = T.trace_beams(P, [0, len(ok)], [om], [1], xp[ok], Np[ok], ds=1e-4, n_steps=12000, psi_grid=GRID,
                            weights=w[ok], traj_stride=stride, deposition="reference", x_launch=pos[ok], s0=s0[ok])
    finally:
        P.set_sched(-1)
    tuples_equal(got[0], want, 46)
    assert results[0]["deposited_power"] == want[4] and 0.0 < want[4] <= 1.0
    assert want[3].max() > 0.0
    assert len(ok) == GRAZING_OK == results[1]["n_ok"]
    g = 46 + ok
    res = m["res"]
    for a, b in ((res.state[g], ref.state), (res.status[g], ref.status), (res.steps[g], ref.steps),
                 (res.P_dep[g], ref.P_dep)):
        assert np.array_equal(a, b)
    assert np.array_equal(res.traj[g], ref.traj, equal_nan=True)
    row = np.zeros(len(GRID))
    row[:-1] = ref.dP_shell[0, :len(GRID) - 1] / P.shell_volumes(GRID)
    assert np.array_equal(m["dP_dV"][1], row) and np.array_equal(got[1][3], row)
    assert results[1]["deposited_power"] == ref.dP_shell[0, len(GRID)]
    assert results[1]["deposited_power"] <= results[1]["w_ok"] * (1 + 1e-12)  # sum w P <= sum w, to rounding
    assert not m["dP_dV"][2].any() and results[2]["deposited_power"] == 0.0


def arrays_equal(a, b):
    assert a["results"] == b["results"]
    for k in ("off", "dP_dV", "pos", "dirs", "w", "entry_status"):
        assert np.array_equal(a[k], b[k]), k
    ok = a["entry_status"] == 0  # (a failed ray's entry point is whatever the entry left)
    for k in ("xp", "Np", "s0"):
        assert np.array_equal(a[k][ok], b[k][ok]), k
    for k in ("state", "status", "steps", "P_dep", "traj"):
        assert np.array_equal(getattr(a["res"], k), getattr(b["res"], k), equal_nan=k in ("state", "traj")), k


def test_second_call_reuses_the_buffers(gpu, T):
    """a handle's second call, with other and fewer launchers, gives what a fresh handle
    gives, and so does a third that grows again: no stale rows, flags or offsets"""
    A, B, C = (new_plasma(T) for _ in range(3))
    first = [LAUNCHERS[0], GRAZING, MISSING, LAUNCHERS[1]]
    second = [MISSING, LAUNCHERS[2], GRAZING]
    a1 = T.solve.make_beams_arrays(A, first, S_MAX, GRID)
    a2 = T.solve.make_beams_arrays(A, second, S_MAX, GRID)
    arrays_equal(a2, T.solve.make_beams_arrays(B, second, S_MAX, GRID))
    assert [r["n_ok"] for r in a2["results"]] == [0, 46, GRAZING_OK]
    a3 = T.solve.make_beams_arrays(A, first, S_MAX, GRID)
    arrays_equal(a3, a1)
    arrays_equal(a3, T.solve.make_beams_arrays(C, first, S_MAX, GRID))


def test_budget_refusal_leaves_the_handle_usable(gpu, T, monkeypatch):
    """The one refusal that comes after the entry has run: the reference deposition's workspace
    of the kept rays against TORJ_WS_GB (read per call).  The call reports it by
    torj_trace_beams' text, and the handle's next call gives what a fresh handle gives."""
    A, B = new_plasma(T), new_plasma(T)
    las = [LAUNCHERS[0], GRAZING]
    monkeypatch.setenv("TORJ_WS_GB", "0.001")  # 1 MiB; 78 kept rays need about 8 MB
    with pytest.raises(T.TorjError, match=r"multi-beam launch: .* for 78 rays .* exceeds the budget"):
        T.solve.make_beams_arrays(A, las, S_MAX, GRID)
    monkeypatch.delenv("TORJ_WS_GB")
    arrays_equal(T.solve.make_beams_arrays(A, las, S_MAX, GRID), T.solve.make_beams_arrays(B, las, S_MAX, GRID))
