"""The block tiny flags of the split pipeline (torj_math.hpp tiny_box_flag,
SplitArgs::tiny_alpha): the trajectory kernel also flags a ray
whose alpha is a zero over the whole block because harmonic 3 is dismissed by
the tiny_alpha bound -- byte 2 / group word 2 beside the exact-zero proof's 1 --
and a wholly flagged group's alpha waves end on the word as before.  No output
bit may move with TORJ_ZBOX_TINY=1 (the default) against 0, counted launches
keep today's path, and the flags fire where they should and nowhere else.

Two test hooks tell the proofs apart: TORJ_TEST_ZFLAG_NAN=s makes the alphas of
a group flagged wholly by the exact-zero proof (word 1) NaN in the blocks from
step s on, as ever; TORJ_TEST_TFLAG_NAN=s does so for word 2.

Shaped like tests/test_gpu_group_flags.py: the 187-ray fan at 92.5 GHz, X mode,
and its copies advanced by the oracle's cold trace, 240 steps in blocks of 20
(each ring slot used three times), chunks of 10.  The advances come from the
oracle's own tau along the fan (it has no tiny skip), per 20-step block:
E, exact zero (d tau == 0); T, tiny (0 < d tau < 1e-100, alpha below 1e-97 m^-1
against tiny_alpha = 1e-20: the tiny-skipped value is 0); A, absorbing (d tau >
1e-12).  Every ray's blocks run E.. T.. A.. in that order.  What the trajectory
kernel then proves over its boxes is confirmed by the hooks on the GPU.

229 rays (3 x 64 + 37): group 0 tiny in every block (T with a block to spare on
either side); group 1 interleaves rays of group 0's kind with absorbing ones,
never flagged: A from the first block on for some, from step 60, 120 and 180 on
for others, so that some ray of it is live and unflagged in every block (the one
group that deposits power: the binned deposition's atomic sums are the same bits
from run to run only then); group 2 exact zeros throughout (the fan advanced by
300 steps: word 1 beside the others' 2); group 3 the 37-ray partial group, tiny
throughout.  129 rays (2 x 64 + 1): group 0 the edge rays, stopped whole at the
first chunk boundary (psi_exit); group 1 goes exact zero -> tiny as the blocks go
by; group 2, one ray, tiny -> absorbing.  (One group going exact zero -> tiny ->
absorbing within 240 steps does not exist on this fan: the oracle's last exact
zero and first absorbing block are 180 steps apart at the least, and the box
proof needs the exact zero to hold 60 steps before the oracle's last one.)"""
import ctypes
import os

import numpy as np
import pytest

from test_gpu_group_flags import BLOCK, CHUNK, DS, GRID, N_STEPS, PSI_EXIT, P_MIN, STRIDE, _bit_equal
from test_gpu_parity import _compare_trace
from test_gpu_split import _fan

pytestmark = pytest.mark.gpu

KNOBS = ("TORJ_ZBOX_TINY", "TORJ_ALPHA_GFLAG", "TORJ_ALPHA_ZFLAG", "TORJ_SPLIT_SERIAL", "TORJ_TRAJ_LDS",
         "TORJ_TINY_ALPHA", "TORJ_ZBOX_LATCH", "TORJ_TEST_ZFLAG_NAN", "TORJ_TEST_TFLAG_NAN")
SCAN = 1600  # steps of the oracle trace the blocks are classified on


class _Env:
    """the knobs of one run set, everything else of KNOBS unset; restored on exit"""

    def __init__(self, T, env):
        self.T, self.env = T, env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.env)
        self.T.abs_Al_init(24)  # TORJ_TINY_ALPHA is read when the table is built

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        self.T.abs_Al_init(24)


@pytest.fixture(scope="module")
def fan(gpu, T, hplasma, oplasma):
    """the fan, the class (0 E, 1 T, 2 A) of each of its rays' 20-step blocks from the
    oracle's tau, and a cache of its cold-advanced copies"""
    pos, xp, Np, s0, w, om = _fan(T, hplasma, n_rings=6, min_az=5)
    assert len(w) == 187
    o = oplasma.trace(xp, Np, om, 1, DS, SCAN, P_min=1e-300, traj_stride=BLOCK)
    assert (o["status"] == T.OK).all()
    tau = np.concatenate([np.zeros((len(w), 1)), o["traj"][:, :, 3]], 1)
    d = np.diff(tau, axis=1)
    cls = np.where(d == 0, 0, np.where(d < 1e-100, 1, 2))
    assert ((d == 0) | (d < 1e-100) | (d > 1e-12)).all() and (np.diff(cls, axis=1) >= 0).all()
    cache = {}

    def at(k):
        if k not in cache:
            if k == 0:
                x, N = xp, Np
            else:
                r = oplasma.trace(xp, Np, om, 1, DS, k, absorption=False)
                assert (r["status"] == T.OK).all() and (r["steps"] == k).all()
                x, N = r["state"][:, :3], r["state"][:, 3:6]
            cache[k] = dict(x=x, N=N, s0=s0 + k * DS, pos=pos, w=w)
        return cache[k]

    return dict(cls=cls, at=at, om=om)


def _first(cls, c):
    """per ray, the first step of its first block of class >= c (a multiple of BLOCK)"""
    return np.array([np.flatnonzero(r >= c)[0] if (r >= c).any() else 10 ** 6 for r in cls]) * BLOCK


def _layout(fan, n):
    """-> the launch's arrays, spec [(advance, ray)], and the kind of each group"""
    cls = fan["cls"]
    t0, a0 = _first(cls, 1), _first(cls, 2)  # where E ends, where A begins
    # tiny throughout [a, a + 240) with a block to spare on either side
    a_t = int(t0.max()) + BLOCK
    tiny = [j for j in range(len(cls)) if a0[j] >= a_t + N_STEPS + BLOCK]
    assert len(tiny) >= 64 + 32 + 37, (a_t, len(tiny))
    # absorbing, at one advance a_a: A from the first block on (a0 <= a_a), or tiny first and A
    # from step 60, 120 or 180 on -- staggered so that some ray is live and unflagged in every
    # block, whichever of them P_min stops on the way
    a_a = 1400
    ab = [j for j in range(len(cls)) if a0[j] <= a_a][:18]
    late = [j for off in (60, 120, 180) for j in [i for i in range(len(cls)) if a0[i] == a_a + off][:5]]
    assert len(ab) == 18 and len(late) >= 14 and all((a0[late] == a_a + off).any() for off in (60, 120, 180))
    if n == 229:
        g0 = [(a_t, j) for j in tiny[:64]]
        g1 = [(a_t, tiny[64 + q // 2]) if q % 2 == 0 else (a_a, (ab + late)[q // 2]) for q in range(64)]
        g2 = [(300, j) for j in range(64)]
        g3 = [(a_t, j) for j in tiny[96:133]]
        spec, kinds = g0 + g1 + g2 + g3, ("tiny", "mixed", "exact", "tiny")
    else:
        # exact zero -> tiny: every ray three blocks before the oracle's last exact zero (the box
        # proof gives up the exact zero 20 to 40 steps before that: block 0 is word 1, the blocks
        # behind it word 2); tiny -> absorbing: one ray 100 steps before its first A block
        g1 = [(int(t0[j]) - 3 * BLOCK, j) for j in range(64)]
        spec = [(0, j) for j in range(64)] + g1 + [(int(a0[ab[0]]) - 100, ab[0])]
        kinds = ("edge", "e_t", "t_a")
    assert len(spec) == n
    out = {f: np.array([fan["at"](k)[f][j] for k, j in spec]) for f in ("x", "N", "s0", "pos", "w")}
    out["spec"], out["kinds"] = spec, kinds
    return out


def _group(c, kind):
    """index arrays of the rays of the groups of this kind"""
    idx = np.arange(len(c["w"]))
    return [idx[64 * g:64 * g + 64] for g, k in enumerate(c["kinds"]) if k == kind]


def _trace(T, hplasma, c, om, deposition="reference"):
    kw = dict(ds=DS, n_steps=N_STEPS, chunk_steps=CHUNK, weights=c["w"], traj_stride=STRIDE, P_min=P_MIN,
              psi_exit=PSI_EXIT, psi_grid=GRID, deposition=deposition)
    if deposition == "reference":
        kw.update(x_launch=c["pos"], s0=c["s0"])
    try:
        hplasma.set_sched(3, BLOCK)
        return T.trace(hplasma, c["x"], c["N"], om, 1, **kw)
    finally:
        hplasma.set_sched(-1)


def _counted(T, hplasma, c, om):
    """a counted launch -> counters, state, status, steps (tests/test_gpu_group_flags.py)"""
    import torch

    n = len(c["w"])
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    x0, N0 = t(c["x"].T), t(c["N"].T)
    state = torch.empty((7, n), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    k = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    cfg = T._lib.TraceCfg(c["om"], 1, DS, N_STEPS, CHUNK, PSI_EXIT, P_MIN, 1, 0)
    stream = torch.cuda.current_stream(dev)
    hplasma.set_sched(3, BLOCK)
    try:
        T._lib.check(T.lib().torj_trace_device(hplasma.handle, cfg, n, x0.data_ptr(), N0.data_ptr(), None, 0, None,
                                               state.data_ptr(), st.data_ptr(), k.data_ptr(), None, None, None,
                                               ctypes.c_void_p(cnt.data_ptr()), stream.cuda_stream))
        T._lib.check(T.lib().torj_trace_check(hplasma.handle, stream.cuda_stream))
    finally:
        hplasma.set_sched(-1)
    return cnt.cpu().numpy(), state.cpu().numpy(), st.cpu().numpy(), k.cpu().numpy()


@pytest.fixture(scope="module", params=[229, 129])
def launch(request, fan):
    c = _layout(fan, request.param)
    c["om"] = fan["om"]
    return c


@pytest.mark.parametrize("tiny", ["1e-20", "0"])
def test_tiny_switch_changes_no_bit(gpu, T, hplasma, launch, tiny):
    """TORJ_ZBOX_TINY=1 against 0: status, steps, state, trajectory samples, P_dep and
    dP_shell are the same bits, serial and overlapped, in the cell, tile and L2
    trajectory kernels, with group words and with per-ray flags, reference and binned
    deposition, latched and unlatched boxes; with tiny_alpha 0 (the exact leg) the new
    flag is off, so both hooks stop the same rays with either setting."""
    c, om = launch, launch["om"]
    for serial in ("0", "1"):
        for lds in ("3", "2", "0"):
            for gflag in ("1", "0"):
                for latch in ("1", "0"):
                    base = {"TORJ_TINY_ALPHA": tiny, "TORJ_SPLIT_SERIAL": serial, "TORJ_TRAJ_LDS": lds,
                            "TORJ_ALPHA_GFLAG": gflag, "TORJ_ZBOX_LATCH": latch}
                    for depo in ("reference", "binned"):
                        out = {}
                        for z in ("1", "0"):
                            with _Env(T, dict(base, TORJ_ZBOX_TINY=z)):
                                out[z] = _trace(T, hplasma, c, om, depo)
                        _bit_equal(out["1"], out["0"], (serial, lds, gflag, latch, depo))
    if tiny == "0":
        for hook in ("TORJ_TEST_ZFLAG_NAN", "TORJ_TEST_TFLAG_NAN"):
            out = {}
            for z in ("1", "0"):
                with _Env(T, {"TORJ_TINY_ALPHA": "0", "TORJ_ZBOX_TINY": z, hook: "0"}):
                    out[z] = _trace(T, hplasma, c, om)
            assert np.array_equal(out["1"].status, out["0"].status) and np.array_equal(out["1"].steps, out["0"].steps)
            assert np.array_equal(out["1"].state, out["0"].state, equal_nan=True)
            if hook == "TORJ_TEST_TFLAG_NAN":
                assert not (out["1"].status == T.NAN).any()


def test_counted_launch_keeps_its_path(gpu, T, hplasma, launch):
    """A counted launch never takes the new flag: all eight counters, state, status and
    steps are equal with the switch on and off, and its stops are the uncounted launch's."""
    c, om = launch, launch["om"]
    cnt = {}
    for z in ("1", "0"):
        with _Env(T, {"TORJ_ZBOX_TINY": z}):
            cnt[z] = _counted(T, hplasma, c, om)
    for k in range(4):
        assert np.array_equal(cnt["1"][k], cnt["0"][k]), (k, cnt["1"][0], cnt["0"][0])
    # ... even under the tiny hook, which a counted launch gives no group to
    with _Env(T, {"TORJ_TEST_TFLAG_NAN": "0"}):
        hooked = _counted(T, hplasma, c, om)
    for k in range(4):
        assert np.array_equal(cnt["1"][k], hooked[k]), k
    with _Env(T, {}):
        g = _trace(T, hplasma, c, om)
    assert np.array_equal(cnt["1"][2], g.status) and np.array_equal(cnt["1"][3], g.steps)


def test_flags_fire_where_they_should(gpu, T, hplasma, launch):
    """Under TORJ_TEST_TFLAG_NAN=s the groups flagged by the tiny proof stop whole at
    the first hooked block with the switch on and nobody stops with it off; under
    TORJ_TEST_ZFLAG_NAN=s the stops are those of the switch off (the exact-zero
    proof's groups, as before this flag existed).  Absorbing and mixed groups never
    stop, the exact-zero group only under the older hook; every ray that does not stop is untouched."""
    c, om = launch, launch["om"]
    n = len(c["w"])
    with _Env(T, {}):
        plain = _trace(T, hplasma, c, om)
    assert not (plain.status == T.NAN).any()
    for s_from in (0, 6 * BLOCK):
        t_on, t_off, z_on, z_off = (None,) * 4
        with _Env(T, {"TORJ_TEST_TFLAG_NAN": str(s_from)}):
            t_on = _trace(T, hplasma, c, om)
        with _Env(T, {"TORJ_TEST_TFLAG_NAN": str(s_from), "TORJ_ZBOX_TINY": "0"}):
            t_off = _trace(T, hplasma, c, om)
        with _Env(T, {"TORJ_TEST_ZFLAG_NAN": str(s_from)}):
            z_on = _trace(T, hplasma, c, om)
        with _Env(T, {"TORJ_TEST_ZFLAG_NAN": str(s_from), "TORJ_ZBOX_TINY": "0"}):
            z_off = _trace(T, hplasma, c, om)
        _bit_equal_nan(t_off, plain)
        _bit_equal_nan(z_on, z_off)
        nan = t_on.status == T.NAN
        print(f"n {n} from step {s_from}: tiny hook stops {int(nan.sum())} rays at steps "
              f"{np.unique(t_on.steps[nan], return_counts=True)}; exact hook {int((z_on.status == T.NAN).sum())}")
        assert (t_on.steps[nan] % BLOCK == 0).all() and (t_on.steps[nan] >= s_from).all()
        for f in ("state", "status", "steps"):
            assert np.array_equal(getattr(t_on, f)[~nan], getattr(plain, f)[~nan]), f
        for g in _group(c, "tiny"):  # the 37-ray partial group included
            assert nan[g].all() and (t_on.steps[g] == s_from).all(), (s_from, t_on.steps[g])
            assert not (z_on.status[g] == T.NAN).any()
        for g in _group(c, "mixed"):
            assert not nan[g].any() and not (z_on.status[g] == T.NAN).any()
        for g in _group(c, "exact"):
            assert not nan[g].any() and (z_on.status[g] == T.NAN).all() and (z_on.steps[g] == s_from).all()
        for g in _group(c, "edge"):  # flagged by the exact proof in block 0, stopped whole at step 10
            assert not nan[g].any()
            assert (z_on.status[g] == T.NAN).all() if s_from == 0 else not (z_on.status[g] == T.NAN).any()
        for g in _group(c, "e_t"):
            # word 1 in block 0, 2 from the block in which the first ray leaves E: the exact hook
            # stops the group whole at step 0 or never, the tiny hook at a later block's first step
            assert (z_on.status[g] == T.NAN).all() if s_from == 0 else not (z_on.status[g] == T.NAN).any()
            assert nan[g].all() and len(set(t_on.steps[g])) == 1
            assert max(s_from, BLOCK) <= t_on.steps[g][0] <= max(s_from, 3 * BLOCK), t_on.steps[g][0]
        for g in _group(c, "t_a"):
            # word 2 in the first blocks, 0 from step 100 on, where the ray absorbs
            assert not (z_on.status[g] == T.NAN).any()
            assert nan[g].all() and (t_on.steps[g] == 0).all() if s_from == 0 else not nan[g].any()
            assert (plain.state[g, 6] > 1e-6).all()


def _bit_equal_nan(a, b):
    for f in ("status", "steps"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in ("state", "P_dep", "dP_shell", "traj"):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f


def test_default_launch_matches_the_oracle(gpu, T, hplasma, oplasma, launch):
    """tests/test_gpu_parity.py _compare_trace's bar on the default launch of both shapes."""
    c, om = launch, launch["om"]
    with _Env(T, {}):
        g = _trace(T, hplasma, c, om, "binned")
    o = oplasma.trace(c["x"], c["N"], om, 1, DS, N_STEPS, chunk_steps=CHUNK, psi_exit=PSI_EXIT, P_min=P_MIN,
                      psi_grid=GRID, weights=c["w"], traj_stride=STRIDE)
    _compare_trace(g, o)
    print(f"n {len(c['w'])}: statuses {np.unique(g.status, return_counts=True)}, tau {g.state[:, 6].min():.3g} - "
          f"{g.state[:, 6].max():.3g}")
