"""The group flag words of the split pipeline (SplitArgs::gflag):
the trajectory kernel writes one word per 64-ray group and ring slot, an alpha
wave of a flagged group ends on it without a load or a store, and the scan
takes the zeros such a wave used to write from the same word.  No output bit
and no counter may move: TORJ_ALPHA_GFLAG=1 (the default) against 0 (the
per-ray flags of round 6) and against TORJ_ALPHA_ZFLAG=0 (no flags at all).

The 92.5 GHz X-mode fan of tests/test_gpu_split.py::test_zero_flags_bit_identical
at small shapes: 20-step blocks (torj_set_sched(p, 3, 20)) over 240 steps, so
each of the four ring slots is used three times, chunks of 10 steps, and rays
built as tests/test_gpu_skip_configs.py builds them -- the fan's rays advanced
by a cold trace of the oracle -- so that the 64-ray groups differ:

  advanced    0  edge rays: alpha exactly 0, psi 0.9967 at step 10, so psi_exit
                 = 0.985 stops every one LEFT_PLASMA at the first chunk boundary
  advanced  300  alpha exactly 0 over all 240 steps (the oracle's alpha is 0 up
                 to step 989 of every ray), psi < 0.91: they run to the end
  advanced  900  steps 900-1140: exact zeros first, then the onset of harmonic 2
                 (first non-zero alpha at steps 989-1048, ray by ray)
  advanced 1200  inside the resonance from the first step (alpha 1e-255 and up)
  advanced 1300  inside it, the strongest absorbers (P_min = 5e-2 stops some)

229 rays (3 x 64 + 37): group 0 flagged in every block (advanced 300), group 1
never (1300), group 2 mixed (300 and 1200 interleaved), group 3 the 37 edge rays,
live and flagged in block 0 and all stopped from block 1 on -- the wave without
a live ray, whose word a skipped write would leave stale from four blocks
earlier.  129 rays (2 x 64 + 1; the last 128-lane alpha workgroup has a wave
with one ray and a wave with none): group 0 the edge rays, group 1 advanced 900
(flagged, then mixed, then unflagged as the blocks go by), group 2 one ray in
the resonance."""
import ctypes
import os

import numpy as np
import pytest

from test_gpu_split import _fan

pytestmark = pytest.mark.gpu

DS, N_STEPS, CHUNK, BLOCK, STRIDE = 1e-4, 240, 10, 20, 10
PSI_EXIT, P_MIN = 0.985, 5e-2
GRID = np.linspace(0, 1, 300)
ADVANCE = (0, 300, 900, 1200, 1300)
KNOBS = ("TORJ_ALPHA_GFLAG", "TORJ_ALPHA_ZFLAG", "TORJ_SPLIT_SERIAL", "TORJ_TRAJ_LDS", "TORJ_TINY_ALPHA",
         "TORJ_TEST_ZFLAG_NAN")
# the three builds of the flags: group words (default), per-ray flags only, none
VARIANTS = {"gflag": {"TORJ_ALPHA_GFLAG": "1"}, "zflag": {"TORJ_ALPHA_GFLAG": "0"}, "none": {"TORJ_ALPHA_ZFLAG": "0"}}


@pytest.fixture(scope="module")
def rays(gpu, T, hplasma, oplasma):
    """the 187-ray fan and its copies advanced by ADVANCE cold steps (the oracle's), once"""
    pos, xp, Np, s0, w, om = _fan(T, hplasma, n_rings=6, min_az=5)
    assert len(w) == 187
    sets = {}
    for k in ADVANCE:
        if k == 0:
            x, N = xp, Np
        else:  # end states of a cold trace are valid start states; s0 grows by k ds
            r = oplasma.trace(xp, Np, om, 1, DS, k, absorption=False)
            assert (r["status"] == T.OK).all() and (r["steps"] == k).all()
            x, N = r["state"][:, :3], r["state"][:, 3:6]
        sets[k] = dict(x=x, N=N, s0=s0 + k * DS, pos=pos, w=w)
    return sets, om


def _pick(sets, spec):
    """rays (advance, index into the fan) -> the arrays of a launch"""
    out = {f: np.array([sets[k][f][j] for k, j in spec]) for f in ("x", "N", "s0", "pos", "w")}
    out["spec"] = spec
    return out


def _layout(sets, n):
    if n == 229:
        mixed = [(300 if j % 2 == 0 else 1200, 64 + j) for j in range(64)]
        spec = [(300, j) for j in range(64)] + [(1300, j) for j in range(64)] + mixed + [(0, j) for j in range(37)]
    else:
        spec = [(0, j) for j in range(64)] + [(900, j) for j in range(64)] + [(1300, 100)]
    assert len(spec) == n
    return _pick(sets, spec)


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


def _trace(T, hplasma, c, om, deposition):
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
    """a counted launch (work words and counters) -> counters, state, status, steps"""
    import torch

    n = len(c["w"])
    dev = torch.device("cuda", 0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    x0, N0 = t(c["x"].T), t(c["N"].T)
    state = torch.empty((7, n), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    k = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.zeros(8, dtype=torch.int64, device=dev)
    cfg = T._lib.TraceCfg(om, 1, DS, N_STEPS, CHUNK, PSI_EXIT, P_MIN, 1, 0)
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


def _bit_equal(a, b, what):
    for f in ("status", "steps", "state", "P_dep", "dP_shell"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)  # (zeros compare as zeros)
    assert np.array_equal(a.traj, b.traj, equal_nan=True), (what, "traj")


@pytest.mark.parametrize("tiny", ["1e-20", "0"])
@pytest.mark.parametrize("n", [229, 129])
def test_group_words_change_no_bit(gpu, T, hplasma, rays, n, tiny):
    sets, om = rays
    c = _layout(sets, n)
    first = None
    for serial in ("0", "1"):
        for lds in ("3", "2", "0"):
            base = {"TORJ_TINY_ALPHA": tiny, "TORJ_SPLIT_SERIAL": serial, "TORJ_TRAJ_LDS": lds}
            for depo in ("reference", "binned"):
                out = {}
                for name, env in VARIANTS.items():
                    with _Env(T, dict(base, **env)):
                        out[name] = _trace(T, hplasma, c, om, depo)
                _bit_equal(out["gflag"], out["zflag"], (serial, lds, depo, "gflag vs zflag"))
                _bit_equal(out["gflag"], out["none"], (serial, lds, depo, "gflag vs none"))
                if first is None:
                    first = out["gflag"]
            cnt = {}
            for name, env in VARIANTS.items():
                with _Env(T, dict(base, **env)):
                    cnt[name] = _counted(T, hplasma, c, om)
            for other in ("zflag", "none"):
                for k in (1, 2, 3):  # state, status, steps
                    assert np.array_equal(cnt["gflag"][k], cnt[other][k]), (serial, lds, other, k)
            # all eight counters: a flagged group's work words are 0 either way
            assert np.array_equal(cnt["gflag"][0], cnt["zflag"][0]), (serial, lds, cnt["gflag"][0], cnt["zflag"][0])
            # without flags the flagged waves are evaluated and count their settled-early
            # harmonics (tests/test_gpu_split.py test_zero_flags_bit_identical)
            assert np.array_equal(cnt["gflag"][0][:7], cnt["none"][0][:7]) and cnt["gflag"][0][7] <= cnt["none"][0][7]
            # the uncounted launch's stops are the counted one's
            assert np.array_equal(cnt["gflag"][2], out["gflag"].status)
            assert np.array_equal(cnt["gflag"][3], out["gflag"].steps)
    # the workload is what the docstring says: the edge rays' group is stopped from the
    # first chunk boundary on, the others' rays run on, some absorbed mid-trace
    g = first
    adv = np.array([k for k, _ in c["spec"]])
    assert (g.status[adv == 0] == T.LEFT_PLASMA).all() and (g.steps[adv == 0] == CHUNK).all()
    assert (g.steps[adv == 300] == N_STEPS).all() and (g.state[adv == 300, 6] == 0.0).all()
    assert (g.state[adv == 1300, 6] > 1.0).any()
    if n == 229:  # (the oracle stops 12 of group 1's rays, at steps 110-180)
        absorbed = g.status == T.ABSORBED
        assert absorbed[64:128].any() and not absorbed[64:128].all() and (g.steps[absorbed] < N_STEPS).any()
    print(f"n {n} tiny {tiny}: statuses {np.unique(g.status, return_counts=True)}")


@pytest.mark.parametrize("n", [229, 129])
def test_nan_hook_stops_the_same_rays(gpu, T, hplasma, rays, n):
    """TORJ_TEST_ZFLAG_NAN=s: the alphas of a wholly flagged group are NaN in the blocks
    that start at step s or later, so its live rays stop NAN at such a block's first
    step -- written by the alpha wave without group words, taken by the scan with them.
    The same rays stop at the same steps either way; some stop (flagged groups occurred)
    and some do not (unflagged ones did)."""
    sets, om = rays
    c = _layout(sets, n)
    adv = np.array([k for k, _ in c["spec"]])
    with _Env(T, {}):
        plain = _trace(T, hplasma, c, om, "reference")
    # a later block's first step: block 6 (its ring slot's second use) for the 229 rays;
    # block 1 for the 129, whose advanced-900 group is provably zero in its first blocks only
    for s_from in (0, 6 * BLOCK if n == 229 else BLOCK):
        out = {}
        for name in ("gflag", "zflag"):
            with _Env(T, dict(VARIANTS[name], TORJ_TEST_ZFLAG_NAN=str(s_from))):
                out[name] = _trace(T, hplasma, c, om, "reference")
        a, b = out["gflag"], out["zflag"]
        assert np.array_equal(a.status, b.status) and np.array_equal(a.steps, b.steps)
        assert np.array_equal(a.state, b.state, equal_nan=True)
        nan = a.status == T.NAN
        print(f"n {n} from step {s_from}: {nan.sum()} of {n} rays stop NAN at steps "
              f"{np.unique(a.steps[nan], return_counts=True)}")
        assert nan.any() and not nan.all()
        assert (a.steps[nan] % BLOCK == 0).all() and (a.steps[nan] >= s_from).all()
        # every other ray is untouched
        for f in ("state", "status", "steps"):
            assert np.array_equal(getattr(a, f)[~nan], getattr(plain, f)[~nan]), f
        # rays in the resonance from the first step sit in groups that are never flagged
        assert not nan[adv >= 1200].any()
        if n == 229:
            # group 0 (alpha exactly 0 throughout, running to the end) stops whole at the
            # first hooked block; group 1 (in the resonance) and the mixed group 2 never
            assert nan[:64].all() and (a.steps[:64] == s_from).all()
            assert not nan[64:192].any()
            # group 3's edge rays: flagged and live in block 0 only
            assert nan[192:].all() if s_from == 0 else not nan[192:].any()
        else:
            # group 0's edge rays as above; group 1 (advanced 900) starts flagged
            assert nan[:64].all() if s_from == 0 else not nan[:64].any()
            assert nan[64:128].all() and (a.steps[64:128] == s_from).all()
