"""The multi-beam calls at the C-ABI boundary (include/torj_hip.h
torj_trace_beams[_device], torj_ray_entry_beams_gpu / _device): the symbols are
exported, and every argument error of beams_plan (csrc/torj_launch.hpp) comes
back through the real library before any device work -- so these run without
a GPU, on a Plasma built on the host."""
import ctypes

import numpy as np
import pytest

OM = 2 * np.pi * 92.5e9
NEW = ("torj_trace_beams", "torj_trace_beams_device", "torj_ray_entry_beams_gpu", "torj_ray_entry_beams_device")


def test_symbols_exported(T):
    L = ctypes.CDLL(T.LIB_PATH)
    for s in NEW:
        assert hasattr(L, s), s
        assert s in T.EXPORTED
    assert T.lib().torj_abi_version() == 8  # symbols added, nothing changed


def rays(n):
    x = np.tile([2.3, 0.0, 0.1], (n, 1))
    N = np.tile([-0.9, 0.0, -0.3], (n, 1))
    return x, N


def err(T, hplasma, counts=(3, 2), **kw):
    """T.trace_beams' error text for these arguments"""
    n = sum(counts)
    off = kw.pop("beam_off", np.concatenate([[0], np.cumsum(counts)]))
    omega = kw.pop("omega", [OM] * len(counts))
    mode = kw.pop("mode", [1] * len(counts))
    kw.setdefault("n_steps", 10)
    x, N = rays(n)
    with pytest.raises(T.TorjError) as e:
        T.trace_beams(hplasma, off, omega, mode, x, N, **kw)
    return str(e.value)


def test_trace_beams_rejections(T, hplasma):
    assert err(T, hplasma, counts=()) == "n_beams must be 1..4096"
    assert err(T, hplasma, counts=(0,) * 4097) == "n_beams must be 1..4096"
    assert err(T, hplasma, counts=(5,), beam_off=[2, 5]) == "beam_off[0] must be 0"
    assert err(T, hplasma, counts=(5, 0, 0), beam_off=[0, 6, 4, 5]) == "beam_off must not decrease (beam 1)"
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert err(T, hplasma, omega=[bad, OM]) == "omega[0] must be finite and > 0"
    assert err(T, hplasma, mode=[1, 0]) == "mode[1] must be +1 (X) or -1 (O)"
    assert err(T, hplasma, n_steps=-1) == "n_steps < 0"
    assert err(T, hplasma, ds=0.0) == "ds must be > 0"
    warm = "absorption must be 0 or 1 in a multi-beam launch (the warm models trace one beam per call)"
    assert err(T, hplasma, absorption="warm_wr") == warm
    assert err(T, hplasma, absorption="warm_fr") == warm
    grid = np.linspace(0, 1, 5)
    fit = "deposition = 1 (reference profile) needs x_launch and s0 (torj_trace_ex)"
    assert err(T, hplasma, psi_grid=grid, deposition="reference") == fit
    assert err(T, hplasma, psi_grid=grid, deposition="reference", s0=np.zeros(5)) == fit
    assert "strictly increasing" in err(T, hplasma, psi_grid=np.array([0.0, 0.5, 0.5, 1.0]))


def raw(T, hplasma, **kw):
    """torj_trace_beams called directly; returns the error text"""
    n = 5
    x, N = (np.ascontiguousarray(a.T) for a in rays(n))
    a = dict(cfg=T._lib.TraceCfg(0.0, 0, 1e-4, 10, 1, 1.0, 1e-6, 1, 0), n_beams=2,
             beam_off=np.array([0, 3, 5], dtype=np.int32), omega=np.array([OM, OM]),
             mode=np.array([1, -1], dtype=np.int32), x0=x, N0=N, state=np.zeros((7, n)),
             status=np.zeros(n, dtype=np.int32), steps=np.zeros(n, dtype=np.int32))
    a.update(kw)
    d, i = T._lib.dptr, T._lib.iptr
    rc = T.lib().torj_trace_beams(hplasma.handle, a["cfg"], a["n_beams"], i(a["beam_off"]), d(a["omega"]),
                                  i(a["mode"]), d(a["x0"]), d(a["N0"]), None, 0, None, None, None, d(a["state"]),
                                  i(a["status"]), i(a["steps"]), None, None, None)
    assert rc != 0
    return T.lib().torj_last_error().decode()


def test_trace_beams_rejections_raw(T, hplasma):
    """what the Python wrapper cannot send: null tables and arrays, the cfg's
    integrator and deposition codes, the handle's sched mode"""
    assert raw(T, hplasma, beam_off=None) == "beam_off is NULL"
    assert raw(T, hplasma, omega=None) == "omega and mode (n_beams each) required"
    assert raw(T, hplasma, state=None) == "x0, N0, state, status, steps required"
    cfg = T._lib.TraceCfg(0.0, 0, 1e-4, 10, 1, 1.0, 1e-6, 1, 0, 2)
    assert raw(T, hplasma, cfg=cfg) == "deposition must be 0 or 1"
    cfg = T._lib.TraceCfg(0.0, 0, 1e-4, 10, 1, 1.0, 1e-6, 1, 0, 0, 1, s_max=1.0)
    assert raw(T, hplasma, cfg=cfg) == \
        "integrator must be 0 in a multi-beam launch (the adaptive integrator traces one beam per call)"
    try:
        for m in (1, 3):
            hplasma.set_sched(m)
            assert raw(T, hplasma) == \
                f"sched mode {m} has no multi-beam form: only the one-shot kernel (torj_set_sched -1, 0, 2)"
    finally:
        hplasma.set_sched(-1)


def test_ray_entry_beams_rejections(T, hplasma):
    x, N = rays(5)
    for kw, text in ((dict(beam_off=[1, 5]), "beam_off[0] must be 0"),
                     (dict(omega=[-OM]), "omega[0] must be finite and > 0"),
                     (dict(mode=[2]), "mode[0] must be +1 (X) or -1 (O)")):
        a = dict(beam_off=[0, 5], omega=[OM], mode=[1])
        a.update(kw)
        with pytest.raises(T.TorjError) as e:
            T.ray_entry_beams(hplasma, a["beam_off"], a["omega"], a["mode"], x, N)
        assert str(e.value) == text


def test_valid_calls_fail_loudly_without_gpu(T, hplasma):
    """No CPU fallback: without a HIP device the valid calls raise."""
    n = ctypes.c_int(0)
    if T.lib().torj_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    x, N = rays(5)
    with pytest.raises(T.TorjError):
        T.trace_beams(hplasma, [0, 3, 5], [OM, 1.1 * OM], [1, -1], x, N, n_steps=10, absorption=False)
    with pytest.raises(T.TorjError):
        T.ray_entry_beams(hplasma, [0, 3, 5], [OM, 1.1 * OM], [1, -1], x, N)
