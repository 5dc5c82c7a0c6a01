"""The trimmed cell-tiled trajectory kernel: the
dead-box latch of traj_run (TORJ_ZBOX_LATCH, read per call) moves no output bit
and no zero flag.  On the fan of test_gpu_split.test_zero_flags_bit_identical
(N_rings 14, min_azimuthal_points 5: a ray count that is no multiple of 64;
3000 steps in chunks of 30 and split blocks of 60, P_min 5e-2 so that rays stop
mid-block), with the tiny-alpha skip and without it.  And the block's last psi,
which eval_one forms where every other step's comes from the next step's
stage-0 sums, is the same bits wherever the block boundaries fall."""
import contextlib
import os

import numpy as np
import pytest

from test_gpu_split import _fan, _run, _trace_counted

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("tiny", ["1e-20", "0"])
def test_zbox_latch_bit_identical(gpu, T, hplasma, tiny):
    """TORJ_ZBOX_LATCH=0 against 1: status, steps, state, trajectory samples
    (NaN-equal), P_dep, dP_shell and the work counters are the same bits -- the
    counters count the alpha evaluations, so equal counters mean the same waves
    were flagged; and under the test hook TORJ_TEST_ZFLAG_NAN=60 (a fully flagged
    wave of a block from step 60 on writes NaN) the same rays stop NAN at the
    same steps either way, so the flags still fire where they did."""
    pos, xp, Np, s0, w, om = _fan(T, hplasma)
    assert len(w) % 64 != 0
    kw = dict(ds=1e-4, n_steps=3000, chunk_steps=30, weights=w, traj_stride=30, P_min=5e-2,
              psi_grid=np.linspace(0, 1, 500), deposition="reference", x_launch=pos, s0=s0)
    out, cnt, hook = {}, {}, {}
    try:
        with _env(TORJ_TINY_ALPHA=tiny):
            T.abs_Al_init(24)  # reads TORJ_TINY_ALPHA
            for z in ("0", "1"):
                with _env(TORJ_ZBOX_LATCH=z):
                    out[z] = _run(T, hplasma, 3, 60, xp, Np, om, 1, **kw)
                    cnt[z] = _trace_counted(T, hplasma, 3, xp, Np, om)
                    with _env(TORJ_TEST_ZFLAG_NAN="60"):
                        hook[z] = _run(T, hplasma, 3, 60, xp, Np, om, 1, **kw)
    finally:
        T.abs_Al_init(24)
    a, b = out["0"], out["1"]
    assert a.status.tolist().count(T.ABSORBED) >= 10, "need mid-trace stops"
    for f in ("status", "steps", "state", "P_dep", "dP_shell"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.traj, b.traj, equal_nan=True)
    assert np.array_equal(cnt["0"], cnt["1"]), (cnt["0"], cnt["1"])
    h0, h1 = hook["0"], hook["1"]
    nan = h0.status == T.NAN
    print(f"tiny_alpha {tiny}: counters {cnt['1']}; flagged waves stop {nan.sum()} of {len(nan)} rays")
    assert nan.sum() >= 64 and (h0.steps[nan] % 60 == 0).all() and (h0.steps[nan] >= 60).all()
    for f in ("status", "steps", "state"):
        assert np.array_equal(getattr(h0, f), getattr(h1, f), equal_nan=True), f


def test_block_end_psi_independent_of_blocks(gpu, T, hplasma):
    """psi at the end of a block's last step comes from eval_one at that point,
    every other step's from the next step's stage-0 sums (cold_step<PSI>): the
    same bits only if both take the same evaluation -- inside the grid the one
    without the Line() extrapolation, decided from cell_axis' delta == 0, which
    holds only while x - clamp(x) is a true difference (contracted with the
    product R = R2 / sqrt(R2) it is that product's rounding error, and the
    extrapolating evaluation then adds it times the slope to psi).  Split blocks
    of 60, 7 and 33 steps put the block ends at different steps: every output is
    the same bits."""
    pos, xp, Np, s0, w, om = _fan(T, hplasma)
    kw = dict(ds=1e-4, n_steps=1500, chunk_steps=30, weights=w, traj_stride=30,
              psi_grid=np.linspace(0, 1, 500), deposition="reference", x_launch=pos, s0=s0)
    a = _run(T, hplasma, 3, 60, xp, Np, om, 1, **kw)
    assert a.P_dep.max() > 0
    for block in (7, 33):
        b = _run(T, hplasma, 3, block, xp, Np, om, 1, **kw)
        for f in ("status", "steps", "state", "P_dep", "dP_shell"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (block, f)
        assert np.array_equal(a.traj, b.traj, equal_nan=True)
