"""The Albajar skip proofs (block zero flags, exact-zero and early settle, the
2^-58 negligible-harmonic skip, the tiny-alpha skip, harmonic 3's dismissal) on
the device away from the 92.5 GHz X-mode fan of the 3 keV tokamak, where
harmonic 2 absorbs and harmonic 3 is always the negligible one:

  A  3 keV  140 GHz X    harmonic 3 absorbs, harmonic 2 absent
  B  3 keV  92.5 GHz O   weak absorption
  C  3 keV  110 GHz X    everything below tiny_alpha
  D  25 keV 92.5 GHz X   every ray ABSORBED mid-trace, harmonics 2 and 3 integrate
  E  25 keV 120 GHz X    down-shifted harmonic 3

Each on 561 rays (= 64 * 8 + 49 = 4 * 140 + 1: ragged at the 64-ray waves of
the split pipeline and at the 4-ray waves of the 16-lane kernel): the 187-ray
fan and the same rays advanced 600 and 1200 cold steps, in built order and
under a seeded permutation that puts rays at different phases of the resonance
crossing into every wave.  Against the oracle (1e-10, statuses and steps exact,
no ray excused), between the schedules, between the two orders, and with every
switch on and off."""
import numpy as np
import pytest

from test_gpu_h3_fast import _with_env
from test_gpu_split import _fan, _run, _trace_counted

pytestmark = pytest.mark.gpu

CFG = {"A": (3e3, 140e9, 1), "B": (3e3, 92.5e9, -1), "C": (3e3, 110e9, 1), "D": (25e3, 92.5e9, 1),
       "E": (25e3, 120e9, 1)}
NAMES = sorted(CFG)
DS, N_STEPS, CHUNK, STRIDE, P_MIN = 1e-4, 3000, 30, 30, 5e-2
GRID = np.linspace(0, 1, 300)
ADVANCE = (600, 1200)
# the permutation's seed: one of those under which every 4-ray group of every
# configuration is staggered (test_workload_is_what_the_table_says asserts it on
# the oracle's tau samples; chosen on the oracle alone: 90, 254, 433 do)
PERM_SEED = 90
WAVES = {3: 60, 2: 0, 0: 0, 1: 3}  # torj_set_sched's second argument: block of 60 steps; 3 waves


class _Ctx:
    def __init__(self, T, plasmas):
        self.T, self.plasmas, self.cfg, self.runs = T, plasmas, {}, {}


@pytest.fixture(scope="module")
def ctx(gpu, T, O, hplasma, oplasma):
    from torj_hip import synthetic as S

    eq = S.circular_tokamak(Te0=25e3)
    hot = (T.Plasma(*S.plasma_args(eq)), O.OraclePlasma(*S.plasma_args(eq)))
    return _Ctx(T, {3e3: (hplasma, oplasma), 25e3: hot})


def _cfg(ctx, name):
    """The 561 rays of a configuration and the oracle's trace of them (built order), once."""
    if name in ctx.cfg:
        return ctx.cfg[name]
    T = ctx.T
    Te0, f, mode = CFG[name]
    hp, op = ctx.plasmas[Te0]
    pos, xp, Np, s0, w, om = _fan(T, hp, mode, n_rings=6, min_az=5, f=f)
    assert len(w) == 187
    X, N, S0 = [xp], [Np], [s0]
    for k in ADVANCE:  # end states of a cold trace are valid start states; s0 grows by k ds
        r = op.trace(xp, Np, om, mode, DS, k, absorption=False)
        assert (r["status"] == T.OK).all() and (r["steps"] == k).all()
        X.append(r["state"][:, :3])
        N.append(r["state"][:, 3:6])
        S0.append(s0 + k * DS)
    c = dict(hp=hp, op=op, mode=mode, om=om, x=np.vstack(X), N=np.vstack(N), s0=np.concatenate(S0),
             pos=np.tile(pos, (3, 1)), w=np.tile(w, 3))
    n = len(c["w"])
    assert n == 561
    c["order"] = {"built": np.arange(n), "perm": np.random.default_rng(PERM_SEED).permutation(n)}
    c["o"] = op.trace(c["x"], c["N"], om, mode, DS, N_STEPS, chunk_steps=CHUNK, psi_grid=GRID, weights=c["w"],
                      traj_stride=STRIDE, P_min=P_MIN, s0=c["s0"])
    ctx.cfg[name] = c
    return c


def _oracle(c, order):
    """the oracle's per-ray results in an order (rays are independent; dP is their sum)"""
    p = c["order"][order]
    o = c["o"]
    return dict(state=o["state"][p], status=o["status"][p], steps=o["steps"][p], Pdep=o["Pdep"][p],
                traj=o["traj"][p], dP=o["dP"])


def _trace(ctx, name, sched, order="perm", env=None, deposition="reference"):
    """One product trace of a configuration, kept for the tests that share it."""
    key = (name, sched, order, tuple(sorted((env or {}).items())), deposition)
    if key not in ctx.runs:
        c = _cfg(ctx, name)
        p = c["order"][order]
        kw = dict(ds=DS, n_steps=N_STEPS, chunk_steps=CHUNK, weights=c["w"][p], traj_stride=STRIDE, P_min=P_MIN,
                  psi_grid=GRID, deposition=deposition, x_launch=c["pos"][p], s0=c["s0"][p])
        fn = lambda: _run(ctx.T, c["hp"], sched, WAVES[sched], c["x"][p], c["N"][p], c["om"], c["mode"], **kw)
        ctx.runs[key] = _with_env(ctx.T, env, fn) if env else fn()
    return ctx.runs[key]


def _errors(g, o):
    """worst x, N (relative to the vector), tau (relative, floored as _compare_trace) and dP errors"""
    from test_gpu_parity import TAU_FLOOR

    gx, ox = g.state, o["state"]
    ex = (np.abs(gx[:, :3] - ox[:, :3]).max(1) / np.linalg.norm(ox[:, :3], axis=1)).max()
    eN = (np.abs(gx[:, 3:6] - ox[:, 3:6]).max(1) / np.linalg.norm(ox[:, 3:6], axis=1)).max()
    et = (np.abs(gx[:, 6] - ox[:, 6]) / np.maximum(np.abs(ox[:, 6]), TAU_FLOOR)).max()
    ed = np.abs(g.dP_shell[:-1] - o["dP"]).max() / max(np.abs(o["dP"]).max(), 1e-300)
    return ex, eN, et, ed


def _bit_equal(a, b, what):
    for f in ("state", "status", "steps", "P_dep", "dP_shell"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)  # (zeros compare as zeros)
    assert np.array_equal(a.traj, b.traj, equal_nan=True), what


@pytest.mark.parametrize("name", NAMES)
def test_parity_with_oracle(ctx, name):
    """The split pipeline (3, blocks of 60 steps), the 16-lane kernel (2), the
    one-lane kernel (0) and the work queue (1, 3 waves) against the oracle in the
    permuted order: _compare_trace's 1e-10 with statuses and steps exact, and the
    binned profile on the 300 shells to 1e-10 of its maximum.  No ray excused:
    under a 2^-45 nudge of the start points the oracle's tau has condition number
    <= 220, so 1e-15 of trajectory agreement predicts <= 2.2e-13."""
    from test_gpu_parity import _compare_trace

    o = _oracle(_cfg(ctx, name), "perm")
    for sched in (3, 2, 0, 1):
        g = _trace(ctx, name, sched, deposition="binned")
        ex, eN, et, ed = _errors(g, o)
        print(f"cfg {name} sched {sched} vs oracle: x {ex:.2e} N {eN:.2e} tau {et:.2e} dP {ed:.2e}")
        _compare_trace(g, o)
        assert np.abs(g.dP_shell[:-1] - o["dP"]).max() <= 1e-10 * max(np.abs(o["dP"]).max(), 1e-300), sched


class _Rays:
    """the per-ray outputs of a trace on a subset of its rays, for _close (the shell profile, a sum
    over all rays, and on request P_dep neutralised, as test_split_equals_fused neutralises what
    it does not compare: the caller asserts them itself)"""

    def __init__(self, r, sel, p_dep=True):
        self.status, self.steps, self.state, self.traj = r.status[sel], r.steps[sel], r.state[sel], r.traj[sel]
        self.P_dep = r.P_dep[sel] if p_dep else np.zeros(int(np.sum(sel)))
        self.dP_shell = np.ones(1)


@pytest.mark.parametrize("name", NAMES)
def test_schedules_agree(ctx, name):
    """Split and 16-lane against the one-lane kernel: the same arithmetic in
    another compilation / with another polynomial length, _close's 1e-12 (P_dep
    1e-9 of the ray's unit power), on all 561 rays, with the binned and with the
    reference deposition.

    One excusal, by a criterion computed from the ray: a ray whose reference
    deposition exceeds what it absorbed (test_ref_depo_gap.ill_posed: started
    inside an absorbing plasma, its dP/ds and psi splines swing through the 0.4 m
    gap back to the launch point; tests/test_ref_depo_gap.py shows the
    reference's own spline missing 1e-9 on exactly these rays under a 3e-14
    nudge) is excused from the P_dep bar, and the leg from the shell profile's,
    where the two runs' x, N differ on that ray.  Where they are the same bits
    nothing is excused; everything else in _close holds for excused rays too.
    Measured: such rays exist in E only (its 187 rays advanced 1200 steps, P_dep
    up to 1.93 of the unit power); E split against one-lane differs on them by up
    to 1.5e-8 (x, N 1e-15 apart), E 16-lane against one-lane (same bits of x, N)
    by 3.6e-12 and nothing is excused, A - D reach at most 2.1e-14 on any ray.
    The switch and order tests hold the same rays' deposition bit for bit."""
    from test_gpu_c3 import _close
    from test_ref_depo_gap import ill_posed, state_eps

    a, ar = _trace(ctx, name, 0, deposition="binned"), _trace(ctx, name, 0)
    ill = ill_posed(ar.P_dep, ar.state[:, 6])
    assert ill.any() == (name == "E"), (name, int(ill.sum()))
    for sched in (3, 2):
        _close(a, _trace(ctx, name, sched, deposition="binned"), 1e-12)
        br = _trace(ctx, name, sched)
        out = ill & (state_eps(ar.state, br.state) > 0)
        d = np.abs(ar.P_dep - br.P_dep)
        print(f"cfg {name} sched {sched} vs 0, reference deposition: {int(ill.sum())} rays deposit more than they "
              f"absorbed (largest P_dep {ar.P_dep.max():.3f}), {int(out.sum())} of them on other bits of x, N; P_dep "
              f"worst {d[~out].max():.2e} on the rays held to 1e-9" +
              (f", {d[out].max():.2e} on the excused" if out.any() else ""))
        if not out.any():
            _close(ar, br, 1e-12)
            continue
        _close(_Rays(ar, ~out), _Rays(br, ~out), 1e-12)
        _close(_Rays(ar, out, p_dep=False), _Rays(br, out, p_dep=False), 1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_order_does_not_matter(ctx, name):
    """The permuted run, un-permuted, against the built-order run, split and
    16-lane: which rays share a wave changes statuses, steps, x, N and the
    trajectory samples by no bit (trajectories do not depend on alpha, a tile is
    bit-identical to its fallback), and tau, P_dep and the samples' tau by 1e-12
    at most (test_lanes_per_ray_bit_identical's form: the Bessel polynomial
    length is chosen per wave)."""
    c = _cfg(ctx, name)
    p = c["order"]["perm"]
    for sched in (3, 2):
        a, b = _trace(ctx, name, sched, "built"), _trace(ctx, name, sched, "perm")
        assert np.array_equal(a.status[p], b.status) and np.array_equal(a.steps[p], b.steps)
        assert np.array_equal(a.state[p, :6], b.state[:, :6])
        rows = [0, 1, 2, 4]
        assert np.array_equal(a.traj[p][:, :, rows], b.traj[:, :, rows], equal_nan=True)
        scale = np.abs(a.state[p]).max(axis=-1) + 1e-300
        et = (np.abs(a.state[p, 6] - b.state[:, 6]) / scale).max()
        assert et <= 1e-12, (sched, et)
        assert np.abs(a.P_dep[p] - b.P_dep).max() <= 1e-12 * max(np.abs(a.P_dep).max(), 1e-300)
        ta, tb = a.traj[p][:, :, 3], b.traj[:, :, 3]
        fin = np.isfinite(ta)
        assert np.array_equal(fin, np.isfinite(tb))
        e_tr = np.abs(ta[fin] - tb[fin]).max()
        assert e_tr <= 1e-12 * np.abs(a.traj[np.isfinite(a.traj)]).max()
        dtau = np.abs(a.state[p, 6] - b.state[:, 6])
        print(f"cfg {name} sched {sched} permuted vs built: tau worst {dtau.max():.2e} absolute, {et:.2e} of the "
              f"ray's state, samples' tau {e_tr:.2e}")


@pytest.mark.parametrize("tiny", ["1e-20", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_zero_flags_bit_identical(ctx, name, tiny):
    """TORJ_ALPHA_ZFLAG=0 against 1 on the split pipeline: no output bit moves."""
    out = {z: _trace(ctx, name, 3, env={"TORJ_ALPHA_ZFLAG": z, "TORJ_TINY_ALPHA": tiny}) for z in ("0", "1")}
    _bit_equal(out["0"], out["1"], (name, tiny))


@pytest.mark.parametrize("sched", [3, 2])
@pytest.mark.parametrize("tiny", ["1e-20", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_h3_fast_bit_identical(ctx, name, tiny, sched):
    """TORJ_H3_FAST=0 against 1, split and 16-lane.  In the 16-lane kernel `work`
    is set on a ray's lane 0 only, so the 60 other lanes of a wave may dismiss
    harmonic 3 among themselves while the 4 writers enter albajar_harmonic<3>:
    right only because a true h3_fast_negligible means that call returns before
    node_sum's shuffle over the ray's 16 lanes.  Configuration A, where harmonic 3
    is the absorbing one, is the case that matters.  The work counters of a
    counted launch in the configuration's mode (_trace_counted: 2000 steps) are
    equal either way: a counted launch sets `work` on every lane that counts, and
    the shortcut is for calls without it, so this pins only that the switch does
    not reach counted launches, as test_h3_fast_counters_unchanged does."""
    out = {on: _trace(ctx, name, sched, env={"TORJ_H3_FAST": on, "TORJ_TINY_ALPHA": tiny}) for on in ("0", "1")}
    _bit_equal(out["0"], out["1"], (name, tiny, sched))
    if tiny == "1e-20":
        c = _cfg(ctx, name)
        p = c["order"]["perm"]
        cnt = {on: _with_env(ctx.T, {"TORJ_H3_FAST": on},
                             lambda: _trace_counted(ctx.T, c["hp"], sched, c["x"][p], c["N"][p], c["om"], c["mode"]))
               for on in ("0", "1")}
        assert np.array_equal(cnt["0"], cnt["1"]), (name, sched, cnt)


@pytest.mark.parametrize("sched", [3, 2])
@pytest.mark.parametrize("tiny", ["1e-20", "0"])
@pytest.mark.parametrize("name", NAMES)
def test_negligible_harmonic_skip_bit_identical(ctx, name, tiny, sched):
    """TORJ_NEGL_SKIP=0 (which also turns the early settle, the zero flags and
    harmonic 3's dismissal off) against 1: no output bit moves; a settled +0
    where the full work gives -0 compares as a zero."""
    out = {on: _trace(ctx, name, sched, env={"TORJ_NEGL_SKIP": on, "TORJ_TINY_ALPHA": tiny}) for on in ("0", "1")}
    _bit_equal(out["0"], out["1"], (name, tiny, sched))


@pytest.mark.parametrize("sched", [3, 2])
@pytest.mark.parametrize("name", NAMES)
def test_tiny_alpha_skip_bounded(ctx, name, sched):
    """What tests/test_gpu_split.py test_tiny_alpha_skip_bounded asserts of the
    traces: statuses, steps, x, N and the samples' positions bit-identical, tau
    within 2 tiny_alpha per metre of ray plus 4e-16 of itself, the deposited
    power likewise.  In C, where every harmonic is below tiny_alpha, the exact
    leg's tau equals the oracle's with no floor (1e-10 relative where tau_cpu > 0:
    test_c3_fan_exact_leg_tau_unfloored's form)."""
    a = _trace(ctx, name, sched, env={"TORJ_H3_FAST": "1", "TORJ_TINY_ALPHA": "0"})
    b = _trace(ctx, name, sched, env={"TORJ_H3_FAST": "1", "TORJ_TINY_ALPHA": "1e-20"})
    for f in ("status", "steps"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.state[:, :6], b.state[:, :6])
    rows = [0, 1, 2, 4]
    assert np.array_equal(a.traj[:, :, rows], b.traj[:, :, rows], equal_nan=True)
    fin = np.isfinite(a.traj[:, :, 3])
    assert np.array_equal(fin, np.isfinite(b.traj[:, :, 3]))
    L = a.steps * DS  # metres of ray traced
    d_tr = np.abs(a.traj[:, :, 3] - b.traj[:, :, 3])
    assert (d_tr[fin] <= 2e-20 * (N_STEPS * DS) + 4e-16 * np.abs(a.traj[:, :, 3])[fin]).all()
    dtau = np.abs(a.state[:, 6] - b.state[:, 6])
    assert (dtau <= 2 * 1e-20 * L + 4e-16 * np.abs(a.state[:, 6])).all(), dtau.max()
    assert np.abs(a.P_dep - b.P_dep).max() <= 1e-12
    # (that test's 1e-12 of the largest shell, for the rounding of a profile of order 1, plus what
    # the skip itself may move: every ray's power by its d tau <= 2 tiny_alpha L, weighted -- in C the
    # exact leg's whole profile is 1.6e-32 and the default leg's is 0)
    w_sum = np.abs(_cfg(ctx, name)["w"]).sum()
    assert np.abs(a.dP_shell - b.dP_shell).max() <= 1e-12 * np.abs(a.dP_shell).max() + 2e-20 * L.max() * w_sum
    print(f"cfg {name} sched {sched}: tau moves by at most {dtau.max():.2e} with tiny_alpha 1e-20")
    if name == "C":
        tc = _oracle(_cfg(ctx, name), "perm")["state"][:, 6]
        pos = tc > 0
        assert pos.sum() > 500
        e = (np.abs(a.state[:, 6] - tc)[pos] / tc[pos]).max()
        print(f"cfg C sched {sched}: exact leg's tau against the oracle's, unfloored: {e:.2e}")
        assert e <= 1e-10, e


def _first_step(tau, th):
    """step of the first trajectory sample with tau > th per ray (never: 10^6)"""
    t = np.nan_to_num(tau)
    return np.where((t > th).any(1), (t > th).argmax(1) * STRIDE + STRIDE, 10 ** 6)


def test_workload_is_what_the_table_says(ctx):
    """On the oracle's own result: A absorbs at harmonic 3 (tau > 1e-2, all OK),
    C stays below 1e-30, D stops every ray ABSORBED; the permutation staggers
    every 4-ray group (the step of first tau > 1e-6 spreads over >= 120 steps, two
    split blocks; in C, where tau never reaches 1e-6, of first tau > 1e-6 of the
    configuration's largest); and the zero flags fire: under TORJ_TEST_ZFLAG_NAN=0
    fully flagged waves stop their rays NAN, >= 64 of them in built order in at
    least one configuration of each plasma."""
    T = ctx.T
    nan = {}
    for name in NAMES:
        c = _cfg(ctx, name)
        o = c["o"]
        tau = o["state"][:, 6]
        print(f"cfg {name}: oracle tau {tau.min():.3g} - {tau.max():.3g}, statuses "
              f"{dict(zip(*np.unique(o['status'], return_counts=True)))}, steps {o['steps'].min()} - {o['steps'].max()}")
        if name == "A":
            assert tau.min() > 1e-2 and (o["status"] == T.OK).all()
        if name == "C":
            assert tau.max() < 1e-30
        if name == "D":
            assert (o["status"] == T.ABSORBED).all()
        tt = o["traj"][:, :, 3]
        th = 1e-6 if np.nanmax(tt) > 1e-6 else 1e-6 * np.nanmax(tt)
        first = _first_step(tt, th)
        share = {}
        for order, p in c["order"].items():
            v = first[p[:560]].reshape(140, 4)
            share[order] = float((v.max(1) - v.min(1) >= 120).mean())
        print(f"cfg {name}: 4-ray groups staggered by >= 120 steps: built {share['built']:.3f}, permuted {share['perm']:.3f}")
        assert share["perm"] == 1.0, (name, share)
        h = _trace(ctx, name, 3, "built", env={"TORJ_TEST_ZFLAG_NAN": "0"})
        nan[name] = int((h.status == T.NAN).sum())
        assert (h.steps[h.status == T.NAN] % WAVES[3] == 0).all()
    print(f"rays stopped NAN by fully flagged waves under the hook, built order: {nan}")
    for Te0 in (3e3, 25e3):
        assert max(nan[k] for k in NAMES if CFG[k][0] == Te0) >= 64, (Te0, nan)
