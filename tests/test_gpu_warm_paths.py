"""Warm absorption traces (absorption 2: weakly, 3: fully relativistic) off the one X2
fan, on every launch path, against the C oracle (oracle/torj_oracle.c RK4 / Tsit5 +
oracle/torj_warm_oracle.c alpha).

The scenarios are those of tests/warm_cases.py (tests/test_warm_cases.py holds the oracle
alone to their table): oblique N_par of either sign, O-mode, Y crossing 1, the shaped
equilibrium with either field direction, points all deferred to k_alpha_warm_big (D) or
partly (E), rays of one wave ABSORBED at differing blocks beside LEFT_PLASMA rays in a
launch with a partial last group (F).  The paths: the library's own plan (the split
pipeline: k_alpha_warm_pts + k_alpha_warm_big), the work-queue kernel's warm instances
(RK4 and the adaptive Tsit5), make_ray(absorption="warm_wr" / "warm_fr").

Bars (the project's, tests/test_gpu_warm.py, tests/test_gpu_c5.py): statuses and step
counts exact; x, N 1e-10 of the vector; tau 1e-9 (model 3) / 1e-8 (model 2) of
max(|tau|, 1e-6), on every ray the oracle's a-priori conditioning flag leaves in (the
flag is worked out only for a launch with a ray beyond the bar -- it costs more than the
trace -- and the CPU file asserts that it leaves every ray of every scenario in); the
saved tau along traj at the same bar of the largest tau.  _check applies them: the
figures of test_gpu_parity.py's _compare_trace, with the warm tau bars where that
function holds tau to the Albajar model's 1e-10.

The fully relativistic queue kernel is latency-bound (one wave: DESIGN.md 3.2), so model 3
takes the queue on A and E only, at 400 steps; B's and F's stops and C's reference
deposition are compared between queue and split with model 2, and against the oracle on
the split path with both."""
import numpy as np
import pytest

import shaped_eq as E
import warm_cases as W
from test_gpu_split import _env_run, _run
from test_launch_plan import DP, GRID, RAYS, S0, TRAJ, XL, H, plan  # noqa: F401  (H: the host build of launch_plan)

pytestmark = pytest.mark.gpu

N_PSI = 300
PSI = np.linspace(0.0, 1.0, N_PSI)
MODELS = [2, 3]
Q3_STEPS = 400  # the fully relativistic model on the queue: A's own count; E's tau is complete by step 300


class _Ctx:
    def __init__(self, T, O):
        self.T, self.O, self.plasmas, self.runs = T, O, {}, {}

    def plasma(self, pk):
        if pk not in self.plasmas:
            self.plasmas[pk] = self.T.Plasma(*W.PLASMAS[pk]())
        return self.plasmas[pk]


@pytest.fixture(scope="module")
def ctx(gpu, T, O):
    return _Ctx(T, O)


def _rays(ctx, key, mode, pk=None):
    """warm_cases.rays, with the product's host entry held to the oracle's (1e-12, every ray OK)"""
    r = W.rays(ctx.O, key, mode, pk)
    if "entered" not in r:
        n = r["n_fan"]
        xp, Np, s0, st = ctx.T.ray_entry(ctx.plasma(r["pk"]), r["pos"][:n], r["dirs"][:n], W.omega(key), mode)
        assert (st == ctx.T.OK).all(), (key, mode, st)
        assert np.abs(xp - r["xp"][:n]).max() < 1e-12 and np.abs(Np - r["Np"][:n]).max() < 1e-12
        assert np.abs(s0 - r["s0"][:n]).max() < 1e-12
        r["entered"] = True
    return r


def _oracle(ctx, key, mode, model, pk=None, n_steps=None, **kw):
    return W.oracle_trace(ctx.O, key, mode, model, pk, n_steps, psi_grid=N_PSI, **kw)


def _gpu(ctx, key, mode, model, leg, pk=None, n_steps=None, deposition="binned", env=None, **kw):
    """One product trace of a scenario, kept for the tests that share it.  leg: "default" the
    library's own plan, "split" sched mode 3 in blocks of 60 steps under env (_env_run),
    "queue" the work-queue kernel (set_sched(1, 0))."""
    r = _rays(ctx, key, mode, pk)
    n_steps = n_steps or W.SCENARIOS[key]["n_steps"]
    k = (key, mode, model, r["pk"], leg, n_steps, deposition, tuple(sorted((env or {}).items())),
         tuple(sorted(kw.items())))
    if k not in ctx.runs:
        hp = ctx.plasma(r["pk"])
        kw = dict(kw, ds=W.DS, n_steps=n_steps, absorption=model, traj_stride=W.STRIDE, psi_grid=PSI,
                  weights=r["w"], deposition=deposition)
        if deposition == "reference":
            kw.update(x_launch=r["pos"], s0=r["s0"])
        args = (r["xp"], r["Np"], W.omega(key), mode)
        if leg == "default":
            hp.set_sched(-1)
            ctx.runs[k] = ctx.T.trace(hp, *args, **kw)
        elif leg == "split":
            ctx.runs[k] = _env_run(ctx.T, hp, env or {}, *args, **kw)
        else:
            ctx.runs[k] = _run(ctx.T, hp, 1, 0, *args, **kw)
    return ctx.runs[k]


def _planned(H, model, n, n_steps, deposition="binned", **kw):  # noqa: F811
    """the launch plan (csrc/torj_launch.hpp launch_plan, host build) of one of this module's calls"""
    has = RAYS | GRID | DP | TRAJ | (XL | S0 if deposition == "reference" else 0)
    return plan(H, absorption=model, n=n, n_psi=N_PSI, has=has, n_steps=n_steps, ds=W.DS, traj_stride=W.STRIDE,
                chunk_steps=max(1, n_steps // 100), deposition=int(deposition == "reference"), **kw)


def _tau_err(g_tau, o_tau):
    return np.abs(g_tau - o_tau) / np.maximum(np.abs(o_tau), W.TAU_FLOOR)


def _check(ctx, what, g, o, key, mode, model, pk=None):
    """The module's bars (its docstring) of a product trace g against the oracle's o; prints
    and returns the measured maxima (x, N, tau, saved tau)."""
    assert np.array_equal(g.status, o["status"]), (what, g.status, o["status"])
    assert np.array_equal(g.steps, o["steps"]), (what, g.steps, o["steps"])
    gs, os_ = g.state, o["state"]
    ex = np.abs(gs[:, :3] - os_[:, :3]).max(1) / np.linalg.norm(os_[:, :3], axis=1)
    eN = np.abs(gs[:, 3:6] - os_[:, 3:6]).max(1) / np.linalg.norm(os_[:, 3:6], axis=1)
    et = _tau_err(gs[:, 6], os_[:, 6])
    # the saved samples both have (before a stop), every ray's up to its last whole stride
    k = o["traj"].shape[1]
    want = np.arange(1, k + 1)[None, :] * W.STRIDE <= o["steps"][:, None]
    assert np.isfinite(g.traj[:, :k, :][want]).all() and np.isfinite(o["traj"][want]).all(), what
    scale = max(np.abs(os_[:, 6]).max(), W.TAU_FLOOR)
    ej = np.where(want, np.abs(g.traj[:, :k, 3] - o["traj"][:, :, 3]), 0.0).max(1) / scale
    exj = np.where(want[:, :, None], np.abs(g.traj[:, :k, :3] - o["traj"][:, :, :3]), 0.0).max()
    bar = W.BAR_TAU[model]
    out = ~((et <= bar) & (ej <= bar))
    keep = np.ones(len(et), bool)
    if out.any():  # the conditioning flag, from the shared trajectory and the algorithm alone
        keep = ~W.flagged(ctx.O, key, mode, model, o, pk)
        print(f"{what}: rays beyond the tau bar {np.flatnonzero(out).tolist()} (tau {et[out]}, saved {ej[out]}); "
              f"flagged rays {np.flatnonzero(~keep).tolist()}")
    print(f"{what}: x {ex.max():.2e} N {eN.max():.2e} tau {et[keep].max():.2e} saved tau {ej[keep].max():.2e} "
          f"(bar {bar:.0e}) saved x {exj:.2e}")
    assert ex.max() <= 1e-10 and eN.max() <= 1e-10, (what, ex.max(), eN.max())
    assert exj <= 3e-10, (what, exj)
    assert keep.mean() >= 0.95, what
    assert et[keep].max() <= bar, (what, et[keep].max())
    assert ej[keep].max() <= bar, (what, ej[keep].max())
    return ex.max(), eN.max(), et[keep].max(), ej[keep].max()


# ------------------------------------------------------------ (a) the library's own plan
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("key,mode", W.PAIRS, ids=W.PAIR_IDS)
def test_default_launch_matches_oracle(ctx, H, key, mode, model):  # noqa: F811
    """Every scenario, mode and model through T.trace as the library plans it -- the split
    pipeline -- against the oracle; B with the default P_min (ABSORBED near step 830) and with
    P_min = 1e-12 (1 000 steps, Y to 1.146)."""
    n, n_steps = len(_rays(ctx, key, mode)["w"]), W.SCENARIOS[key]["n_steps"]
    assert _planned(H, model, n, n_steps)["path"] == H.SPLIT
    g, o = _gpu(ctx, key, mode, model, "default"), _oracle(ctx, key, mode, model)
    _check(ctx, f"(a) {key} mode {mode:+d} model {model} default", g, o, key, mode, model)
    if key == "B":
        assert (o["status"] == W.ABSORBED).all()
        g, o = _gpu(ctx, key, mode, model, "default", P_min=1e-12), _oracle(ctx, key, mode, model, P_min=1e-12)
        assert (o["status"] == W.OK).all()
        _check(ctx, f"(a) B mode {mode:+d} model {model} default, P_min 1e-12", g, o, key, mode, model)


# ------------------------------------------------------------ (b) the deferred list
def _counted(ctx, key, mode, model):
    """the work counters of a counted split launch of a scenario (torj_trace_device with a
    counters array): ray-steps, alpha calls, ..., [6] sum lrm, [7] sum lrm^2 (torj_hip/flops.py)"""
    import ctypes

    import torch

    T, r = ctx.T, _rays(ctx, key, mode)
    hp, n, n_steps = ctx.plasma(r["pk"]), len(r["w"]), W.SCENARIOS[key]["n_steps"]
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    x0, N0 = t(r["xp"].T), t(r["Np"].T)
    state = torch.empty((7, n), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    k = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    cfg = T._lib.TraceCfg(W.omega(key), mode, W.DS, n_steps, max(1, n_steps // 100), 1.0, 1e-6, model, 0)
    stream = torch.cuda.current_stream(dev)
    hp.set_sched(3, 0)
    try:
        T._lib.check(T.lib().torj_trace_device(hp.handle, cfg, n, x0.data_ptr(), N0.data_ptr(), None, 0, None,
                                               state.data_ptr(), st.data_ptr(), k.data_ptr(), None, None, None,
                                               ctypes.c_void_p(cnt.data_ptr()), stream.cuda_stream))
        T._lib.check(T.lib().torj_trace_check(hp.handle, stream.cuda_stream))
    finally:
        hp.set_sched(-1)
    return cnt.cpu().numpy(), state.cpu().numpy().T, st.cpu().numpy(), k.cpu().numpy()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("key,mode", [("D", 1), ("D", -1), ("E", 1)], ids=["D-X", "D-O", "E-X"])
def test_deferred_list(ctx, key, mode, model):
    """TORJ_WARM_DEFER_LRM=0 (every point through the list and k_alpha_warm_big) gives the
    default split's bits in D (where every point is deferred anyway) and in E (where waves are
    partly deferred), and both meet the oracle.  The work counters of a counted launch (model
    2: the scan decodes the weakly relativistic work words) say which kernel took the points:
    with lrm in 1..5, sum (lrm - 4)(lrm - 5) = 0 exactly when every point has lrm 4 or 5 (D:
    only deferred points), > 0 when some point has lrm <= 3 (undeferred), and
    sum lrm (lrm - 3) > 0 only when some point has lrm >= 4 (deferred)."""
    a = _gpu(ctx, key, mode, model, "split", deposition="reference")
    b = _gpu(ctx, key, mode, model, "split", deposition="reference", env={"TORJ_WARM_DEFER_LRM": "0"})
    for f in ("state", "status", "steps", "P_dep", "dP_shell"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.traj, b.traj, equal_nan=True)
    _check(ctx, f"(b) {key} mode {mode:+d} model {model} split, blocks of 60", a, _oracle(ctx, key, mode, model),
           key, mode, model)
    if model != 2:
        return
    cnt, state, st, steps = _counted(ctx, key, mode, model)
    n, n_steps = len(st), W.SCENARIOS[key]["n_steps"]
    calls, sl, sl2 = int(cnt[1]), int(cnt[6]), int(cnt[7])
    print(f"(b) {key} mode {mode:+d} model 2: counters {cnt}; mean lrm {sl / calls:.3f}")
    assert (st == W.OK).all() and cnt[0] == n * n_steps and calls == 4 * n * n_steps
    assert _tau_err(state[:, 6], a.state[:, 6]).max() <= W.BAR_TAU[model]  # the counted kernel instances
    assert calls <= sl <= 5 * calls
    if key == "D":
        assert sl2 - 9 * sl + 20 * calls == 0, cnt
    else:
        assert sl2 - 9 * sl + 20 * calls > 0 and sl2 - 3 * sl > 0, cnt


# ------------------------------------------------------------ (c) the work-queue kernel
QUEUE = [(k, m, 2, None) for k, m in W.PAIRS] + [("A", 1, 3, Q3_STEPS), ("A", -1, 3, Q3_STEPS), ("E", 1, 3, Q3_STEPS)]


@pytest.mark.parametrize("key,mode,model,n_steps", QUEUE,
                         ids=[f"{k}-{'X' if m == 1 else 'O'}-{md}" for k, m, md, _ in QUEUE])
def test_queue_kernel_matches_oracle(ctx, H, key, mode, model, n_steps):  # noqa: F811
    """set_sched(1, 0): the warm instances of the RK4 work-queue kernel against the oracle."""
    n = len(_rays(ctx, key, mode)["w"])
    assert _planned(H, model, n, n_steps or W.SCENARIOS[key]["n_steps"], sched_mode=1)["path"] == H.QUEUE
    g, o = _gpu(ctx, key, mode, model, "queue", n_steps=n_steps), _oracle(ctx, key, mode, model, n_steps=n_steps)
    if key == "A" and mode == 1:
        assert o["state"][:, 6].min() > 1.0
    _check(ctx, f"(c) {key} mode {mode:+d} model {model} queue", g, o, key, mode, model)


# ------------------------------------------------------------ (d) stops
@pytest.mark.parametrize("key,mode", [("B", -1), ("F", 1)], ids=["B-O", "F-X"])
def test_stops_split_and_queue(ctx, H, key, mode):  # noqa: F811
    """Mid-block stops against the oracle: B's ABSORBED rays (default P_min) and F's 68 rays
    (the fan ABSORBED at differing steps, two rays LEFT_PLASMA, the last group partial), on
    the split path with both models and on the queue with model 2; the NaN pattern of the
    trajectory samples past a stop equal between the paths.  F also in batches of 64 rays
    (TORJ_SPLIT_BATCH=64: 64 + 4): the unbatched launch's bits."""
    T = ctx.T
    for model in MODELS:
        assert _planned(H, model, len(_rays(ctx, key, mode)["w"]), W.SCENARIOS[key]["n_steps"])["path"] == H.SPLIT
        o = _oracle(ctx, key, mode, model)
        g = _gpu(ctx, key, mode, model, "default")
        _check(ctx, f"(d) {key} model {model} split", g, o, key, mode, model)
        st = g.status.tolist()
        if key == "F":
            assert T.ABSORBED in st and T.LEFT_PLASMA in st
            assert len(st) == 68 and len(np.unique(g.steps[g.status == T.ABSORBED])) >= 4
        else:
            assert st.count(T.ABSORBED) == len(st) and g.steps.max() < W.SCENARIOS[key]["n_steps"]
        # past a stop the samples are NaN
        k = g.traj.shape[1]
        past = np.arange(1, k + 1)[None, :] * W.STRIDE > g.steps[:, None]
        assert past.any() and np.isnan(g.traj[past]).all() and np.isfinite(g.traj[~past]).all()
        if model == 2:
            q = _gpu(ctx, key, mode, model, "queue")
            _check(ctx, f"(d) {key} model {model} queue", q, o, key, mode, model)
            assert np.array_equal(np.isfinite(g.traj), np.isfinite(q.traj))
        if key == "F":
            s = _gpu(ctx, key, mode, model, "split")
            b = _gpu(ctx, key, mode, model, "split", env={"TORJ_SPLIT_BATCH": "64"})
            for f in ("state", "status", "steps", "P_dep"):
                assert np.array_equal(getattr(s, f), getattr(b, f)), (model, f)
            assert np.array_equal(s.traj, b.traj, equal_nan=True)
            # binned shells are fp64 atomics: their order differs between launches
            assert np.abs(s.dP_shell - b.dP_shell).max() <= 1e-13 * np.abs(s.dP_shell).max()
            _check(ctx, f"(d) F model {model} split in batches of 64", b, o, key, mode, model)


# ------------------------------------------------------------ (e) deposition
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("key,mode", [p for p in W.PAIRS if p[0] in "AC"],
                         ids=[i for i, p in zip(W.PAIR_IDS, W.PAIRS) if p[0] in "AC"])
def test_deposition(ctx, key, mode, model):
    """The binned shell profile of the default launch against the oracle's dP per shell, at the
    model's tau bar of the profile's maximum (dP is w times a difference of P = exp(-tau), so
    its error is linear in tau's); dP_shell[-1] against sum w P_dep; and the reference
    deposition between queue and split at 1e-9 (test_split_warm_equals_fused's bar) -- model 3
    at 400 steps (C's X-mode tau is above 1 there in the oracle)."""
    r = _rays(ctx, key, mode)
    g, o = _gpu(ctx, key, mode, model, "default"), _oracle(ctx, key, mode, model)
    scale = np.abs(o["dP"]).max()
    ed = np.abs(g.dP_shell[:-1] - o["dP"]).max() / scale
    ep = np.abs(g.P_dep - o["Pdep"]).max() / o["Pdep"].max()
    es = abs(g.dP_shell[-1] - np.dot(r["w"], g.P_dep)) / g.dP_shell[-1]
    n_steps = Q3_STEPS if model == 3 else None
    if model == 3 and mode == 1:
        assert _oracle(ctx, key, mode, model, n_steps=n_steps)["state"][:, 6].min() > 1.0
    a = _gpu(ctx, key, mode, model, "queue", n_steps=n_steps, deposition="reference")
    b = _gpu(ctx, key, mode, model, "split", n_steps=n_steps, deposition="reference")
    eq = np.abs(a.P_dep - b.P_dep).max()
    er = np.abs(a.dP_shell - b.dP_shell).max() / np.abs(a.dP_shell).max()
    print(f"(e) {key} mode {mode:+d} model {model}: binned dP vs oracle {ed:.2e} of max, P_dep {ep:.2e}, "
          f"dP_shell[-1] vs sum w P_dep {es:.2e}; reference, queue vs split: P_dep {eq:.2e} dP_shell {er:.2e}")
    assert scale > 0 and ed <= W.BAR_TAU[model], ed
    assert ep <= W.BAR_TAU[model], ep
    assert es <= 1e-12, es
    assert np.array_equal(a.status, b.status) and np.array_equal(a.steps, b.steps)
    assert np.abs(a.dP_shell).max() > 0 and eq <= 1e-9 and er <= 1e-9, (eq, er)


# ------------------------------------------------------------ (f) the adaptive integrator
AD = dict(s_max=0.3, n_chunks=15)
AD_CAP = 400  # accepted-step capacity


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("mode", [-1, 1], ids=["O", "X"])
def test_adaptive_matches_oracle(ctx, H, mode, model):  # noqa: F811
    """A with integrator="adaptive" (Tsit5, dtmax = ds = 1e-3, default tolerances, 0.3 m in 15
    chunks from the entry's s0): the warm instances of the adaptive queue kernel.

    O-mode: the oracle takes exactly 300 steps per ray, all dtmax-limited: this module's bars,
    step counts exact, arc lengths to 1e-12.

    X-mode: the controller is error-limited through the layer (the oracle: 300 - 303 steps, ds
    down to 1e-4 and below), so test_adaptive_step_control_engaged's rule holds: statuses
    equal, >= 75 % of the rays with the oracle's count, |d steps| <= 2; same-count rays to
    1e-9 in x, N and ten times the model's fixed-step bar in tau (the factor that test grants
    x and N for the step sizes' rounding); the other rays to 1e-5 = 10 reltol (the controller's
    RMS norm runs over seven components).  Every saved P = exp(-tau) is >= 0 (the power clamp
    of the reference's ContinuousCallback, fed by a warm alpha)."""
    T, key = ctx.T, "A"
    r = _rays(ctx, key, mode)
    n = len(r["w"])
    p = plan(H, absorption=model, n=n, has=RAYS | S0 | TRAJ, n_steps=AD_CAP, ds=W.DS, traj_stride=1, integrator=1,
             chunk_steps=4, **AD)
    assert (p["path"], p["adaptive"]) == (H.QUEUE, 1)
    hp = ctx.plasma(r["pk"])
    hp.set_sched(-1)
    g = T.trace(hp, r["xp"], r["Np"], W.omega(key), mode, ds=W.DS, n_steps=AD_CAP, integrator="adaptive", s0=r["s0"],
                absorption=model, traj_stride=1, **AD)
    o = W.oracle_trace(ctx.O, key, mode, model, n_steps=AD_CAP, integrator=1, s0="entry", traj_stride=1, **AD)
    bar = W.BAR_TAU[model]
    what = f"(f) A mode {mode:+d} model {model} adaptive"
    assert np.array_equal(g.status, o["status"]) and (o["status"] == T.OK).all()
    saved = np.arange(AD_CAP)[None, :] < g.steps[:, None]
    P = np.exp(-g.traj[:, :, 3])
    assert np.isfinite(g.traj[saved]).all() and (P[saved] >= 0.0).all() and (np.exp(-g.state[:, 6]) >= 0).all()
    gs, os_ = g.state, o["state"]
    ex = np.abs(gs[:, :6] - os_[:, :6]).max(1) / np.abs(os_[:, :6]).max(1)
    et = _tau_err(gs[:, 6], os_[:, 6])
    if mode == -1:
        assert (o["steps"] == 300).all() and np.array_equal(g.steps, o["steps"])
        es = np.abs(g.traj[:, :300, 4] - o["traj"][:, :300, 4]).max()
        ej = np.abs(g.traj[:, :300, 3] - o["traj"][:, :300, 3]).max() / os_[:, 6].max()
        e3x, e3N, _ = E.trace_errs(gs, os_, W.TAU_FLOOR)
        print(f"{what}: 300 steps on every ray; x {e3x:.2e} N {e3N:.2e} tau {et.max():.2e} saved tau {ej:.2e} "
              f"(bar {bar:.0e}) arc lengths {es:.2e}")
        assert e3x <= 1e-10 and e3N <= 1e-10 and et.max() <= bar and ej <= bar and es <= 1e-12
        return
    assert 300 <= o["steps"].min() and o["steps"].max() <= 303 and o["steps"].max() > 300
    same = g.steps == o["steps"]
    sg = np.concatenate([r["s0"][:, None], g.traj[:, :, 4]], 1)
    so = np.concatenate([r["s0"][:, None], o["traj"][:, :, 4]], 1)
    assert np.nanmin(np.diff(so, axis=1)) < 0.5 * W.DS  # genuinely error-limited
    print(f"{what}: oracle steps {o['steps'].tolist()}, GPU {g.steps.tolist()}")
    assert same.mean() >= 0.75 and np.abs(g.steps - o["steps"]).max() <= 2
    print(f"{what}: same count {same.mean():.2f}: x, N {ex[same].max():.2e} tau {et[same].max():.2e} (bars 1e-9, "
          f"{10 * bar:.0e}); "
          + (f"other rays: x, N {ex[~same].max():.2e} tau {et[~same].max():.2e} (bar 1e-5)" if (~same).any()
             else "no other rays"))
    miss = np.flatnonzero(same & ~((ex <= 1e-9) & (et <= 10 * bar)))
    report = [(int(i), float(ex[i]), float(et[i]), np.diff(sg[i, :g.steps[i] + 1]).tolist(),
               np.diff(so[i, :o["steps"][i] + 1]).tolist()) for i in miss[:2]]
    assert miss.size == 0, ("same-count rays beyond the bars: (ray, x/N, tau, GPU ds, oracle ds)", report)
    assert ex.max() <= 1e-5 and et.max() <= 1e-5, (ex.max(), et.max())


@pytest.mark.parametrize("model", MODELS)
def test_adaptive_power_clamp_with_a_warm_alpha(ctx, model):
    """(f) leaves the clamp idle (alpha ds <= 0.07 there).  warm_cases.CLAMP on B -- dtmax 2 cm
    through the fundamental, loose tolerances, after test_adaptive_power_clamp -- makes Tsit5
    overshoot P below zero: every saved P is >= 0 and none is NaN, the clamp engaged (saved
    P = 0, as in the oracle: tests/test_warm_cases.py), and the statuses are the oracle's."""
    T, c = ctx.T, W.CLAMP
    r = _rays(ctx, "B", -1)
    hp = ctx.plasma(r["pk"])
    hp.set_sched(-1)
    g = T.trace(hp, r["xp"], r["Np"], W.omega("B"), -1, ds=c["ds"], n_steps=W.CLAMP_CAP, integrator="adaptive",
                s0=r["s0"], absorption=model, traj_stride=1, s_max=c["s_max"], n_chunks=c["n_chunks"],
                abstol=c["abstol"], reltol=c["reltol"])
    o = W.oracle_trace(ctx.O, "B", -1, model, n_steps=W.CLAMP_CAP, **c)
    saved = np.arange(W.CLAMP_CAP)[None, :] < g.steps[:, None]
    P = np.exp(-g.traj[:, :, 3])
    Po = np.exp(-o["traj"][:, :, 3])[np.arange(W.CLAMP_CAP)[None, :] < o["steps"][:, None]]
    print(f"(f) B model {model} adaptive, dtmax 2 cm: statuses {g.status.tolist()} steps {g.steps.tolist()} (oracle "
          f"{o['steps'].tolist()}), saved P = 0: {(P[saved] == 0).sum()} (oracle {(Po == 0).sum()})")
    assert not np.isnan(g.traj[saved]).any()
    assert (P[saved] >= 0.0).all() and (P[saved] == 0.0).any() and (Po == 0.0).any()
    assert (np.exp(-g.state[:, 6]) >= 0).all()
    assert np.array_equal(g.status, o["status"]) and T.ABSORBED in g.status.tolist()


# ------------------------------------------------------------ (g) make_ray
@pytest.mark.parametrize("absorption,integrator,ds", [("warm_wr", "rk4", 1e-3), ("warm_wr", "adaptive", 1e-4),
                                                      ("warm_fr", "rk4", 1e-3)])
def test_make_ray_warm(ctx, absorption, integrator, ds):
    """make_ray(absorption="warm_wr" / "warm_fr") on A's central ray (X-mode, 0.4 m: through the
    layer), after test_adaptive_reference_deposition_and_make_ray: dP_dV and the deposited
    power against deposition_ref.power_deposition_profile over the oracle's samples, at the
    model's bar of the profile's maximum.  Fixed steps of 1e-3 (A's); the adaptive leg at
    dtmax 1e-4, where the steps are dtmax-limited and the counts exact."""
    import deposition_ref as D
    from torj_hip import synthetic as S

    T, O, s = ctx.T, ctx.O, S.SETUP
    model = T.solve.ABSORPTION[absorption]
    bar = W.BAR_TAU[model]
    hp, op = ctx.plasma("circ"), W.oracle_plasma(O, "circ")
    N0 = T.pol_tor_angles_2_vector(s["steering_angle_pol"], np.deg2rad(W.SCENARIOS["A"]["tor"]))
    x0 = np.array([s["R0"], 0.0, s["z0"]])
    f, s_max = W.SCENARIOS["A"]["f"], 0.4
    om = 2 * np.pi * f
    hp.set_sched(-1)
    sv, u, P_beam, dP_dV, pdep = T.make_ray(hp, x0, N0, f, 1, s_max, PSI, ds=ds, integrator=integrator,
                                            absorption=absorption)
    st, xp, Np, s0 = op.ray_entry(x0, N0, om, 1)
    assert st == 0
    n_steps = int(round(s_max / ds))
    if integrator == "adaptive":
        o = op.trace(xp[None], Np[None], om, 1, ds, 2 * n_steps + 400, samples=True, traj_stride=1, integrator=1,
                     s_max=s_max, s0=[s0], absorption=model)
    else:
        o = op.trace(xp[None], Np[None], om, 1, ds, n_steps, samples=True, traj_stride=1, s0=[s0], absorption=model)
    k = int(o["steps"][0])
    assert o["status"][0] == 0 and o["state"][0, 6] > 1.0 and len(sv) == k + 2
    assert np.abs(sv[2:] - o["traj"][0, :k, 4]).max() <= 1e-12
    assert np.abs(u[2:] - o["traj"][0, :k, :3]).max() < 1e-9
    et = np.abs(-np.log(P_beam[-1]) - o["state"][0, 6]) / o["state"][0, 6]
    svr, psi, dpds = D.ray_vectors(x0, s0, ds, k, o["samples"][0], op.evaluate("psi", x0))
    prof, P = D.power_deposition_profile(svr, psi, dpds, PSI, op.volume)
    ed = np.abs(dP_dV - prof).max() / np.abs(prof).max()
    ep = abs(pdep - P) / P
    print(f"(g) make_ray {absorption} {integrator} ds {ds:g}: {k} steps, tau {o['state'][0, 6]:.3f} ({et:.2e}), "
          f"dP_dV {ed:.2e} of max, P_dep {P:.6f} ({ep:.2e}); bar {bar:.0e}")
    assert P > 0.5 and np.abs(prof).max() > 0
    assert ed <= bar and ep <= bar, (ed, ep)


# ------------------------------------------------------------ (h) B -> -B, no second implementation
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("mode", [1, -1], ids=["X", "O"])
def test_field_reversal(ctx, mode, model):
    """C through the reversed field against C, on the GPU alone: the warm alpha takes N_par
    signed, and N_par changes sign with B; the trace must not."""
    a, b = _gpu(ctx, "C", mode, model, "default"), _gpu(ctx, "C", mode, model, "default", pk="s-")
    assert np.array_equal(a.status, b.status) and np.array_equal(a.steps, b.steps)
    ex, eN, et = E.trace_errs(b.state, a.state, W.TAU_FLOOR)
    bits = all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("state", "P_dep"))
    print(f"(h) C mode {mode:+d} model {model}, B -> -B on the GPU: x {ex:.2e} N {eN:.2e} tau {et:.2e}; "
          f"bit-identical: {bits}")
    assert a.state[:, 6].min() > 0.2
    assert ex <= 1e-10 and eN <= 1e-10 and et <= W.BAR_TAU[model], (ex, eN, et)
    _check(ctx, f"(h) C reversed mode {mode:+d} model {model} default", b, _oracle(ctx, "C", mode, model, pk="s-"),
           "C", mode, model, "s-")
