"""Harmonic 3 dismissed from the prologue's outputs (torj_math.hpp
h3_fast_negligible, GLTable::h3_fast, env TORJ_H3_FAST read by abs_Al_init) on
the device: a wave skips harmonic 3 only when every lane that reaches it is
provably skipped by albajar_harmonic<3> itself, so no output bit moves, and
counted launches never take the shortcut, so the work counters stay put."""
import os

import numpy as np
import pytest

from test_gpu_split import _fan, _run, _trace_counted

pytestmark = pytest.mark.gpu


def _with_env(T, env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    T.abs_Al_init(24)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        T.abs_Al_init(24)


@pytest.mark.parametrize("sched", [3, 2, 0])
@pytest.mark.parametrize("tiny", ["1e-20", "0"])
def test_h3_fast_bit_identical(gpu, T, hplasma, tiny, sched):
    """TORJ_H3_FAST=0 against 1 on the inputs of test_zero_flags_bit_identical,
    split (3) and fused (2: sixteen lanes per ray; 0: one), with the tiny-alpha
    skip and without it: below the second harmonic the exact leg integrates
    harmonic 3, so waves there mix integrating and dismissible lanes -- the case
    the all-or-nothing rule is for.  The one-lane fused kernels never take the
    shortcut: ray_segment always passes `work` there, and the shortcut is for
    calls without it, so the 0 leg pins only that fact.  In the 16-lane kernels
    `work` is set on a ray's lane 0 alone and the shortcut is live on the other
    15 (tests/test_gpu_skip_configs.py: where harmonic 3 is the absorbing one)."""
    pos, xp, Np, s0, w, om = _fan(T, hplasma)
    kw = dict(ds=1e-4, n_steps=3000, chunk_steps=30, weights=w, traj_stride=30, P_min=5e-2,
              psi_grid=np.linspace(0, 1, 500), deposition="reference", x_launch=pos, s0=s0)
    out = {}
    for on in ("0", "1"):
        out[on] = _with_env(T, {"TORJ_H3_FAST": on, "TORJ_TINY_ALPHA": tiny},
                            lambda: _run(T, hplasma, sched, 60, xp, Np, om, 1, **kw))
    a, b = out["0"], out["1"]
    assert a.status.tolist().count(T.ABSORBED) >= 10, "need mid-trace stops"
    for f in ("state", "status", "steps", "P_dep", "dP_shell"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.traj, b.traj, equal_nan=True)


def test_h3_fast_counters_unchanged(gpu, T, hplasma):
    """Counted launches take albajar_harmonic's own path whatever the switch:
    all eight work counters equal, split and fused."""
    pos, xp, Np, s0, w, om = _fan(T, hplasma)
    for sched in (3, 0):
        c = {on: _with_env(T, {"TORJ_H3_FAST": on}, lambda: _trace_counted(T, hplasma, sched, xp, Np, om))
             for on in ("0", "1")}
        assert np.array_equal(c["0"], c["1"]), (sched, c)
