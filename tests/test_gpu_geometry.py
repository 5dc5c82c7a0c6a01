"""Trace parity off the one equilibrium and the one launch the other GPU tests use.

Every other GPU trace test runs on synthetic.circular_tokamak() -- psi an exact
quadratic without a cross term, up-down symmetric, hR == hZ -- from SETUP's launch
point on the low-field side at phi = 0.  Here: the shaped equilibrium of
tests/shaped_eq.py (40 x 61 nodes, hR != hZ, a mixed derivative, shifted and
asymmetric in Z, either field direction), launched into from the low-field side
below the midplane, from the top and from the high-field side, each also rotated
about the Z axis by 2.3 rad so that |y| is comparable to |x| or larger, both modes, and a 25 keV plasma on
which harmonics 2 and 3 both integrate.  187-ray fans (n_rings 6, min_az 5: ragged
at 64 and at 4 rays per wave), 92.5 GHz, 6 000 steps of 1e-4 m, termination checks
every 60 steps, blocks of 60 on the split path, 200 shells.

Against the oracle: _compare_trace's bars (x, N, tau 1e-10, statuses and steps
exact), the binned shell profile and the rays' deposited power to 1e-10 of their
maxima, on the split path with every trajectory kernel (TORJ_TRAJ_LDS 0..3), the
sixteen-lane kernel, the one-lane kernel and the work queue; the reference
deposition between the schedules (_close, 1e-12) and against FITPACK; the tiled
kernels bit-identical to their global-memory fallback.  And the physics' exact
symmetries, which need no second implementation (an error the oracle shares is
invisible to parity): rotation about Z, reversal of the field, and the mirror image
on the circular tokamak, whose mirrored fan drives the tiles' lower-half cell
indices from below.  tests/test_oracle_symmetry.py holds the oracle to the same
symmetries on CPU; the discrepancies of both are printed side by side."""
from types import SimpleNamespace

import numpy as np
import pytest

import shaped_eq as E
from test_gpu_beams_plasmas import _Beam, per_ray_equal, sched_all
from test_gpu_c3 import _close
from test_gpu_parity import _compare_trace
from test_gpu_split import _env_run, _run, _trace_counted
from test_oracle_symmetry import ENTRY_PHIS, oracle_entry
from test_split_plan_gflag import H, traj_mode  # noqa: F401  (H: the host build of the split plan)

pytestmark = pytest.mark.gpu

DS, N_STEPS, CHUNK, STRIDE = 1e-4, 6000, 60, 1000
GRID = np.linspace(0.0, 1.0, 200)
KW = dict(ds=DS, n_steps=N_STEPS, chunk_steps=CHUNK, traj_stride=STRIDE)
WAVES = {2: 0, 0: 0, 1: 3}  # torj_set_sched's second argument (the work queue: 3 waves)
SPLIT = [("split", str(m)) for m in range(4)]  # blocks of 60 steps, TORJ_TRAJ_LDS = m
SCHEDS = [("sched", 0), ("sched", 1)]
# plasma, launch, mode, rotation
CASES = [("s+", name, mode, phi) for name in sorted(E.LAUNCHES) for mode in (1, -1) for phi in (0.0, E.PHI_ROT)]
CASES += [("hot", "lfs_down", 1, 0.0), ("hot", "lfs_down", 1, E.PHI_ROT)]
IDS = [f"{p}-{n}-{'X' if m == 1 else 'O'}-{'rot' if phi else 'phi0'}" for p, n, m, phi in CASES]
PLASMAS = {"s+": dict(sigma=1.0), "s-": dict(sigma=-1.0), "hot": dict(Te0=25e3)}


class _Ctx:
    def __init__(self, T, O):
        self.T, self.O, self.plasmas, self.cfg, self.runs = T, O, {}, {}, {}

    def plasma(self, key):
        if key not in self.plasmas:
            args = E.shaped_args(**PLASMAS[key])
            self.plasmas[key] = (self.T.Plasma(*args), self.O.OraclePlasma(*args))
        return self.plasmas[key]


@pytest.fixture(scope="module")
def ctx(gpu, T, O):
    return _Ctx(T, O)


def _cfg(ctx, case, oracle=True):
    """One case's fan, its entry into the case's plasma (the condition of every launch
    here: the oracle's entry status is 0 for every ray) and the oracle's trace, once."""
    if case not in ctx.cfg:
        T = ctx.T
        pk, name, mode, phi = case
        hp, op = ctx.plasma(pk)
        pos, dirs, w = E.fan(T, E.LAUNCHES[name], 6, 5, phi)
        assert len(w) == 187
        st, xo, No, s0o = oracle_entry(op, pos, dirs, mode)
        assert (st == 0).all(), (case, st)
        xp, Np, s0, sth = T.ray_entry(hp, pos, dirs, E.OMEGA, mode)
        assert (sth == T.OK).all(), (case, sth)
        assert np.abs(xp - xo).max() < 1e-12 and np.abs(Np - No).max() < 1e-12
        ctx.cfg[case] = dict(hp=hp, op=op, mode=mode, pos=pos, dirs=dirs, w=w, xp=xp, Np=Np, s0=s0)
    c = ctx.cfg[case]
    if oracle and "o" not in c:
        c["o"] = c["op"].trace(c["xp"], c["Np"], E.OMEGA, c["mode"], DS, N_STEPS, chunk_steps=CHUNK, psi_grid=GRID,
                               weights=c["w"], traj_stride=STRIDE)
    return c


def _gpu(ctx, case, leg, deposition="binned", env=None):
    """One product trace of a case, kept for the tests that share it.  leg: ("split", m) the
    split path in blocks of 60 steps with TORJ_TRAJ_LDS = m, or ("sched", s) torj_set_sched(s)."""
    key = (case, leg, deposition, tuple(sorted((env or {}).items())))
    if key not in ctx.runs:
        c = _cfg(ctx, case, oracle=False)
        kw = dict(KW, psi_grid=GRID, weights=c["w"], deposition=deposition)
        if deposition == "reference":
            kw.update(x_launch=c["pos"], s0=c["s0"])
        args = (c["xp"], c["Np"], E.OMEGA, c["mode"])
        if leg[0] == "split":
            ctx.runs[key] = _env_run(ctx.T, c["hp"], dict(env or {}, TORJ_TRAJ_LDS=leg[1]), *args, **kw)
        else:
            ctx.runs[key] = _run(ctx.T, c["hp"], leg[1], WAVES[leg[1]], *args, **kw)
    return ctx.runs[key]


def _errors(g, o):
    """worst x, N, tau (_compare_trace's figures), shell profile and P_dep errors against the oracle"""
    ex, eN, et = E.trace_errs(g.state, o["state"])
    ed = np.abs(g.dP_shell[:-1] - o["dP"]).max() / max(np.abs(o["dP"]).max(), 1e-300)
    ep = np.abs(g.P_dep - o["Pdep"]).max() / max(o["Pdep"].max(), 1e-300)
    return ex, eN, et, ed, ep


def test_lds_leg_runs_k_traj_lds(ctx, H):  # noqa: F811
    """The TORJ_TRAJ_LDS=1 legs below run k_traj_lds, not its fallback k_traj: the plan of
    this module's launches (187 rays, 6 000 steps) on this module's grid says so.  On the
    129 x 129 grid the same setting falls back to the L2 kernel."""
    hp, _ = ctx.plasma("s+")
    assert (len(hp.R_coords), len(hp.Z_coords)) == (E.NR, E.NZ) == (40, 61)
    assert traj_mode(H, 187, E.NR, E.NZ, "1") == (1, 42 * 63 * 48)
    assert traj_mode(H, 187, 129, 129, "1")[0] == 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_with_oracle(ctx, case):
    """Every trajectory kernel of the split path, the one-lane kernel and the work queue
    with the binned deposition (the oracle's), the sixteen-lane kernel with the reference
    deposition (with the binned one the plan takes one lane per ray)."""
    c = _cfg(ctx, case)
    o = c["o"]
    print(f"{case}: oracle statuses {dict(zip(*np.unique(o['status'], return_counts=True)))}, steps "
          f"{o['steps'].min()} - {o['steps'].max()}, tau {o['state'][:, 6].min():.3g} - {o['state'][:, 6].max():.3g}")
    for leg in SPLIT + SCHEDS:
        g = _gpu(ctx, case, leg)
        ex, eN, et, ed, ep = _errors(g, o)
        print(f"{case} {leg} vs oracle: x {ex:.2e} N {eN:.2e} tau {et:.2e} dP {ed:.2e} P_dep {ep:.2e}")
        _compare_trace(g, o)
        assert ed <= 1e-10 and ep <= 1e-10, (leg, ed, ep)
        assert abs(g.dP_shell[-1] - np.sum(c["w"] * o["Pdep"])) <= 1e-10 * max(o["Pdep"].max(), 1e-300)
        fin = (np.isfinite(o["traj"]) & np.isfinite(g.traj))[:, :, :3]  # the samples both have (before a stop)
        assert fin[:, 0].all()
        assert np.abs(g.traj[:, :, :3][fin] - o["traj"][:, :, :3][fin]).max() < 3e-10
    g = _gpu(ctx, case, ("sched", 2), "reference")
    ex, eN, et = E.trace_errs(g.state, o["state"])
    print(f"{case} ('sched', 2) vs oracle: x {ex:.2e} N {eN:.2e} tau {et:.2e}")
    _compare_trace(g, o)
    if case[0] == "hot":
        # every ray is absorbed mid-trace, and harmonics 2 and 3 both integrate: the work
        # counters (2 000 steps, before any ray stops) hold more harmonic integrals than
        # points with absorption, so some points integrated two harmonics
        assert (o["status"] == ctx.T.ABSORBED).all() and o["steps"].max() < N_STEPS
        cnt = _trace_counted(ctx.T, c["hp"], 3, c["xp"], c["Np"], E.OMEGA, c["mode"])
        print(f"{case}: work counters {cnt}")
        assert cnt[3] > cnt[2] > 0, cnt


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_deposition_schedules_agree(ctx, case):
    """The reference deposition (the FITPACK walk over make_ray's samples): every schedule
    against the one-lane kernel at _close's bars (1e-12; P_dep 1e-9 of the ray's unit
    power), each against the oracle's trace, and where the beam deposits (the low-field-side
    launches) five rays' P_dep against power_deposition_profile restated on FITPACK, at
    test_c3_fan_reference_deposition_vs_fitpack's bar."""
    import deposition_ref as D

    c = _cfg(ctx, case)
    a = _gpu(ctx, case, ("sched", 0), "reference")
    _compare_trace(a, c["o"])
    for leg in SPLIT + [("sched", 2), ("sched", 1)]:
        b = _gpu(ctx, case, leg, "reference")
        _compare_trace(b, c["o"])
        _close(a, b, 1e-12)
        print(f"{case} {leg} vs one lane, reference deposition: P_dep {np.abs(a.P_dep - b.P_dep).max():.2e}, "
              f"dP {np.abs(a.dP_shell - b.dP_shell).max() / max(np.abs(a.dP_shell).max(), 1e-300):.2e} of max")
    if case[1] != "lfs_down":
        return
    idx = np.linspace(0, 186, 5).astype(int)
    o = c["op"].trace(c["xp"][idx], c["Np"][idx], E.OMEGA, c["mode"], DS, N_STEPS, chunk_steps=CHUNK, samples=True,
                      s0=c["s0"][idx])
    assert np.array_equal(o["steps"], a.steps[idx])
    for k, i in enumerate(idx):
        sv, psi, dpds = D.ray_vectors(c["pos"][i], c["s0"][i], DS, o["steps"][k], o["samples"][k],
                                      c["op"].evaluate("psi", c["pos"][i]))
        _, P = D.power_deposition_profile(sv, psi, dpds, GRID, c["op"].volume)
        for r in (a, _gpu(ctx, case, ("split", "3"), "reference")):
            assert abs(r.P_dep[i] - P) <= 1e-11 * P + 2e-20 * DS * o["steps"][k], (i, r.P_dep[i], P)


@pytest.mark.parametrize("tile,cap", [("2", "30"), ("3", "2")])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tiles_bit_identical_to_fallback(ctx, case, tile, cap):
    """k_traj_tile / k_traj_cell with the tile's margin at 0 (rays leave their tile
    mid-block), with a small cap (some waves untiled) and with no tile at all: the bits of
    the plain run (test_traj_tile_bit_identical_to_global_fallback, on this grid)."""
    ref = _gpu(ctx, case, ("split", tile), "reference")
    for env in ({"TORJ_TILE_MARGIN": "0"}, {"TORJ_TILE_CAP": cap}, {"TORJ_TILE_CAP": "0"}):
        r = _gpu(ctx, case, ("split", tile), "reference", env)
        for f in ("state", "status", "steps", "P_dep", "dP_shell"):
            assert np.array_equal(getattr(ref, f), getattr(r, f)), (env, f)
        assert np.array_equal(ref.traj, r.traj, equal_nan=True), env


def test_gpu_entry_matches_host_and_oracle(ctx):
    """k_ray_entry against the host entry and the oracle's on the three launches and the
    launch of the entry finding (shaped_eq.EDGE_LAUNCH), at phi = 0, 2.3 and six more
    toroidal angles, both modes, at test_gpu_ray_entry_matches_host_and_oracle's bars, every
    ray against the oracle; no ray fails to enter at any angle, in any of the three."""
    T = ctx.T
    hp, op = ctx.plasma("s+")
    for name, launch in sorted(dict(E.LAUNCHES, edge=E.EDGE_LAUNCH).items()):
        for phi in ENTRY_PHIS[:8]:
            pos, dirs, _w = E.fan(T, launch, 6, 5, phi)
            for mode in (1, -1):
                g = T.ray_entry(hp, pos, dirs, E.OMEGA, mode, gpu=True)
                h = T.ray_entry(hp, pos, dirs, E.OMEGA, mode)
                so, xo, No, s0o = oracle_entry(op, pos, dirs, mode)
                assert np.array_equal(g[3], h[3]) and np.array_equal(g[3], so), (name, phi, mode)
                assert (g[3] == T.OK).all(), (name, phi, mode, g[3])
                for a, b in zip(g[:3], h[:3]):
                    assert np.abs(a - b).max() < 1e-12
                assert np.abs(g[0] - xo).max() < 1e-12 and np.abs(g[1] - No).max() < 1e-12
                assert np.abs(g[2] - s0o).max() < 1e-12


def _symmetry(what, a, b, state_b, oa, ob, ostate_b):
    """b's trace, its end states brought into a's frame, against a's at _compare_trace's bars
    with the shell profile and P_dep to 1e-10 of their maxima; the oracle's own discrepancy
    between its two traces beside it"""
    e = E.trace_errs(state_b, a.state)
    ed = np.abs(a.dP_shell - b.dP_shell).max() / max(np.abs(a.dP_shell).max(), 1e-300)
    ep = np.abs(a.P_dep - b.P_dep).max() / max(np.abs(a.P_dep).max(), 1e-300)
    line = f"{what}: GPU x {e[0]:.2e} N {e[1]:.2e} tau {e[2]:.2e} dP {ed:.2e} P_dep {ep:.2e}"
    if oa is not None:
        eo = E.trace_errs(ostate_b, oa["state"])
        line += (f" | oracle x {eo[0]:.2e} N {eo[1]:.2e} tau {eo[2]:.2e} dP "
                 f"{np.abs(oa['dP'] - ob['dP']).max() / max(np.abs(oa['dP']).max(), 1e-300):.2e}")
    print(line)
    _compare_trace(SimpleNamespace(state=state_b, status=b.status, steps=b.steps),
                   dict(state=a.state, status=a.status, steps=a.steps))
    assert ed <= 1e-10 and ep <= 1e-10, (what, ed, ep)


@pytest.mark.parametrize("pk,name,mode", [c[:3] for c in CASES if c[3] == 0.0],
                         ids=[i[:-5] for i, c in zip(IDS, CASES) if c[3] == 0.0])
def test_rotation_invariance(ctx, pk, name, mode):
    """The launch rotated about Z by 2.3 rad, its result rotated back, against the unrotated
    one: exact in the physics, so only rounding separates them (the oracle's own: <= 4.3e-14
    in x, N, 1e-12 in tau)."""
    ca, cb = (pk, name, mode, 0.0), (pk, name, mode, E.PHI_ROT)
    oa, ob = _cfg(ctx, ca)["o"], _cfg(ctx, cb)["o"]
    xb = _cfg(ctx, cb)["xp"]
    assert (np.abs(xb[:, 1]) > 0.9 * np.abs(xb[:, 0])).all()  # |y| comparable to |x|, or larger
    for leg in (("split", "3"), ("split", "2"), ("split", "1"), ("sched", 0)):
        a, b = _gpu(ctx, ca, leg), _gpu(ctx, cb, leg)
        _symmetry(f"rotation {pk} {name} {mode:+d} {leg}", a, b, E.rot_state(b.state, -E.PHI_ROT), oa, ob,
                  E.rot_state(ob["state"], -E.PHI_ROT))
        fin = np.isfinite(a.traj)
        assert np.array_equal(fin, np.isfinite(b.traj))
        back = np.concatenate([E.rotz(b.traj[:, :, :3], -E.PHI_ROT), b.traj[:, :, 3:]], 2)
        assert np.abs(back[fin] - a.traj[fin]).max() < 3e-10


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "s+"], ids=[i for i, c in zip(IDS, CASES) if c[0] == "s+"])
def test_field_reversal(ctx, case):
    """The plasma with B -> -B gives the same trace: the dispersion and the Albajar
    absorption depend on |B| and N_par^2."""
    rev = ("s-",) + case[1:]
    ca, cb = _cfg(ctx, case), _cfg(ctx, rev)
    assert np.abs(ca["xp"] - cb["xp"]).max() < 1e-12 and np.abs(ca["Np"] - cb["Np"]).max() < 1e-12
    for leg in (("split", "3"), ("split", "2"), ("split", "1"), ("sched", 0)):
        a, b = _gpu(ctx, case, leg), _gpu(ctx, rev, leg)
        _symmetry(f"reversal {case[1:]} {leg}", a, b, b.state, ca["o"], cb["o"], cb["o"]["state"])
    # and the reversed plasma against the oracle's trace of it and of the plasma it reverses
    _compare_trace(_gpu(ctx, rev, ("split", "3")), cb["o"])
    _compare_trace(_gpu(ctx, rev, ("split", "3")), ca["o"])


@pytest.mark.parametrize("mode", [1, -1])
def test_mirror_on_circular(ctx, T, O, hplasma, oplasma, mode):
    """On circular_tokamak() (box and psi symmetric in Z) SETUP's fan mirrored in Z = 0,
    traced through the plasma's mirror image (B is a pseudovector: the toroidal field
    reversed, tests/test_oracle_symmetry.py), gives the mirrored trace, with the node tile
    and the cell tile: their lower-half cell indices, driven from below; and against the
    oracle's trace of the mirrored fan."""
    from torj_hip import synthetic as S

    s = S.SETUP
    setup = ((s["R0"], 0.0, s["z0"]), np.rad2deg(s["steering_angle_pol"]), np.rad2deg(s["steering_angle_tor"]))
    image = S.plasma_args(E.mirror_image(S.circular_tokamak()))
    hm = T.Plasma(*image)
    pos, dirs, w = E.fan(T, setup, 6, 5)
    runs = {}
    for key, hp, p, d in (("up", hplasma, pos, dirs), ("down", hm, E.mirror(pos), E.mirror(dirs))):
        xp, Np, s0, st = T.ray_entry(hp, p, d, E.OMEGA, mode, gpu=True)
        assert (st == T.OK).all()
        kw = dict(KW, psi_grid=GRID, weights=w)
        runs[key] = {lds: _env_run(T, hp, {"TORJ_TRAJ_LDS": lds}, xp, Np, E.OMEGA, mode, **kw) for lds in ("2", "3")}
        runs[key]["xp"], runs[key]["Np"] = xp, Np
    assert (runs["down"]["xp"][:, 2] < 0).all() and (runs["up"]["xp"][:, 2] > 0).all()
    oa = oplasma.trace(runs["up"]["xp"], runs["up"]["Np"], E.OMEGA, mode, DS, N_STEPS, chunk_steps=CHUNK,
                       psi_grid=GRID, weights=w)
    ob = O.OraclePlasma(*image).trace(runs["down"]["xp"], runs["down"]["Np"], E.OMEGA, mode, DS, N_STEPS,
                                      chunk_steps=CHUNK, psi_grid=GRID, weights=w)
    for lds in ("2", "3"):
        a, b = runs["up"][lds], runs["down"][lds]
        _symmetry(f"mirror SETUP {mode:+d} TORJ_TRAJ_LDS={lds}", a, b, E.mirror_state(b.state), oa, ob,
                  E.mirror_state(ob["state"]))
        _compare_trace(b, ob)
        assert np.abs(b.dP_shell[:-1] - ob["dP"]).max() <= 1e-10 * np.abs(ob["dP"]).max()


# launch, mode, rotation, rays taken from the 187-ray fan, plasma (0 shaped, 1 shaped reversed, 2 circular)
BEAMS = (("lfs_down", 1, 0.0, 46, 0), ("top", -1, E.PHI_ROT, 5, 1), ("hfs", 1, 0.0, 13, 1),
         ("lfs_down", -1, E.PHI_ROT, 46, 1), ("setup", 1, 0.0, 1, 2), ("top", 1, 0.0, 13, 0),
         ("setup", -1, E.PHI_ROT, 13, 2), ("hfs", -1, E.PHI_ROT, 0, 0))


def test_beams_plasmas_mix_the_launches(ctx, T, hplasma, oplasma):
    """One trace_beams(plasmas=) call over [shaped, shaped reversed, circular] with eight
    beams that mix the launches, their rotations and both modes (46 + 5 + 13 + 46 + 1 + 13 +
    13 + 0 rays): the bits of one launch per beam on its plasma with sixteen lanes and with
    one lane per ray (reference deposition, the rows of dP_shell included), and on the
    automatic path with the binned deposition each beam against the oracle of its plasma."""
    from torj_hip import synthetic as S

    s = S.SETUP
    launches = dict(E.LAUNCHES, setup=((s["R0"], 0.0, s["z0"]), 30.0, 0.0))
    hs = [ctx.plasma("s+")[0], ctx.plasma("s-")[0], hplasma]
    ops = [ctx.plasma("s+")[1], ctx.plasma("s-")[1], oplasma]
    b = dict(pos=[], w=[], xp=[], Np=[], s0=[])
    off, mode, bp = [0], [], []
    for name, m, phi, k, j in BEAMS:
        pos, dirs, w = E.fan(T, launches[name], 6, 5, phi)
        xp, Np, s0, st = T.ray_entry(hs[j], pos, dirs, E.OMEGA, m)
        assert (st == T.OK).all(), (name, m, phi, j)
        for key, v in (("pos", pos), ("w", w), ("xp", xp), ("Np", Np), ("s0", s0)):
            b[key].append(v[:k])
        off.append(off[-1] + k), mode.append(m), bp.append(j)
    b = {k: np.concatenate(v) for k, v in b.items()}
    omega = [E.OMEGA] * len(BEAMS)
    ref = dict(psi_grid=GRID, deposition="reference")

    def multi(**kw):
        return T.trace_beams(hs[0], off, omega, mode, b["xp"], b["Np"], **KW, weights=b["w"], plasmas=hs,
                             beam_plasma=bp, **kw)

    for lanes in (16, 1):
        try:
            sched_all(hs, 2 if lanes == 16 else 0)
            m = multi(x_launch=b["pos"], s0=b["s0"], **ref)
            for k in range(len(BEAMS)):
                sl = slice(off[k], off[k + 1])
                if sl.start == sl.stop:
                    assert not m.dP_shell[k].any()
                    continue
                one = T.trace(hs[bp[k]], b["xp"][sl], b["Np"][sl], E.OMEGA, mode[k], **KW, weights=b["w"][sl],
                              x_launch=b["pos"][sl], s0=b["s0"][sl], **ref)
                per_ray_equal(m, sl, one)
                assert np.array_equal(m.dP_shell[k], one.dP_shell), (lanes, k)
        finally:
            sched_all(hs, -1)
    m = multi(psi_grid=GRID, deposition="binned")
    for k in range(len(BEAMS)):
        sl = slice(off[k], off[k + 1])
        if sl.start == sl.stop:
            continue
        o = ops[bp[k]].trace(b["xp"][sl], b["Np"][sl], E.OMEGA, mode[k], DS, N_STEPS, chunk_steps=CHUNK,
                             psi_grid=GRID, weights=b["w"][sl])
        ex, eN, et = E.trace_errs(m.state[sl], o["state"])
        ed = np.abs(m.dP_shell[k, :-1] - o["dP"]).max() / max(np.abs(o["dP"]).max(), 1e-300)
        print(f"beam {k} {BEAMS[k]} vs oracle: x {ex:.2e} N {eN:.2e} tau {et:.2e} dP {ed:.2e}")
        _compare_trace(_Beam(m, sl), o)
        assert ed <= 1e-10
        assert np.abs(m.P_dep[sl] - o["Pdep"]).max() <= 1e-10 * max(o["Pdep"].max(), 1e-300)
