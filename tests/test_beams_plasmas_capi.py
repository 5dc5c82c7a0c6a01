"""The multi-beam calls through differing plasmas at the C-ABI boundary
(include/torj_hip.h torj_trace_beams_plasmas[_device],
torj_ray_entry_beams_plasmas_gpu / _device): the symbols are exported, and every
argument error the plasma form adds (beams_plasmas_plan, csrc/torj_launch.hpp)
comes back through the real library before any device work, naming the argument
or its index -- so these run without a GPU, on Plasmas built on the host."""
import ctypes

import numpy as np
import pytest

OM = 2 * np.pi * 92.5e9
NEW = ("torj_trace_beams_plasmas", "torj_trace_beams_plasmas_device", "torj_ray_entry_beams_plasmas_gpu",
       "torj_ray_entry_beams_plasmas_device")


@pytest.fixture(scope="module")
def plasmas(T):
    """Three plasmas on device 0 (two of differing temperature and density, one on another
    grid) and one built for device 1."""
    from torj_hip import synthetic as S

    eqs = (S.circular_tokamak(), S.circular_tokamak(Te0=6000, ne_scale=0.6),
           S.circular_tokamak(nR=72, nZ=64, R_range=(0.9, 2.7), Z_range=(-0.9, 0.9), Te0=1500))
    on0 = [T.Plasma(*S.plasma_args(eq)) for eq in eqs]
    return on0, T.Plasma(*S.plasma_args(eqs[0]), device=1)


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


def err(T, p, listed, beam_plasma, counts=(3, 2), **kw):
    """T.trace_beams' error text for these arguments"""
    n = sum(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    kw.setdefault("n_steps", 10)
    x, N = rays(n)
    with pytest.raises(T.TorjError) as e:
        T.trace_beams(p, off, [OM] * len(counts), [1] * len(counts), x, N, plasmas=listed, beam_plasma=beam_plasma,
                      **kw)
    return str(e.value)


def test_trace_rejections(T, plasmas):
    (a, b, c), far = plasmas
    assert err(T, a, [], [0, 0]) == "n_plasmas must be 1..4096"
    assert err(T, a, [a] * 4097, [0, 0]) == "n_plasmas must be 1..4096"
    assert err(T, a, [a, None, c], [0, 2]) == "plasmas[1] is NULL"
    assert err(T, a, [a, b, c], [0, -1]) == "beam_plasma[1] = -1 is outside 0..2 (n_plasmas = 3)"
    assert err(T, a, [a, b, c], [3, 0]) == "beam_plasma[0] = 3 is outside 0..2 (n_plasmas = 3)"
    # another device is refused whether or not a beam uses that plasma, from either side
    cross = "plasmas[2] is on device 1, the launching handle on device 0 (one device per launch)"
    assert err(T, a, [a, b, far], [0, 1]) == cross
    assert err(T, far, [far, a], [0, 0]) == \
        "plasmas[1] is on device 0, the launching handle on device 1 (one device per launch)"
    # refused as in every multi-beam launch
    warm = "absorption must be 0 or 1 in a multi-beam launch (the warm models trace one beam per call)"
    assert err(T, a, [a, b], [0, 1], absorption=2) == warm
    try:
        for m in (1, 3):
            a.set_sched(m)  # the launching handle's knob
            assert err(T, a, [b, c], [0, 1]) == \
                f"sched mode {m} has no multi-beam form: only the one-shot kernel (torj_set_sched -1, 0, 2)"
    finally:
        a.set_sched(-1)
    # the other three tables: beams_tables_check's messages
    with pytest.raises(T.TorjError, match=r"omega\[1\] must be finite and > 0"):
        x, N = rays(5)
        T.trace_beams(a, [0, 3, 5], [OM, -OM], [1, 1], x, N, n_steps=10, plasmas=[a, b], beam_plasma=[0, 1])


def raw(T, p, **kw):
    """torj_trace_beams_plasmas called directly; returns the error text"""
    n = 5
    x, N = (np.ascontiguousarray(a.T) for a in rays(n))
    a = dict(cfg=T._lib.TraceCfg(0.0, 0, 1e-4, 10, 1, 1.0, 1e-6, 1, 0), n_plasmas=2, plasmas=[p, p],
             beam_plasma=np.array([0, 1], dtype=np.int32))
    a.update(kw)
    off, om, md = np.array([0, 3, 5], dtype=np.int32), np.array([OM, OM]), np.array([1, -1], dtype=np.int32)
    state, status, steps = np.zeros((7, n)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    d, i = T._lib.dptr, T._lib.iptr
    rc = T.lib().torj_trace_beams_plasmas(p.handle, a["n_plasmas"], T._lib.handles(a["plasmas"]), i(a["beam_plasma"]),
                                          a["cfg"], 2, i(off), d(om), i(md), d(x), d(N), None, 0, None, None, None,
                                          d(state), i(status), i(steps), None, None, None)
    assert rc != 0
    return T.lib().torj_last_error().decode()


def test_trace_rejections_raw(T, plasmas):
    """what the Python wrapper cannot send: the null tables, the cfg's integrator code"""
    (a, _, _), _ = plasmas
    assert raw(T, a, plasmas=None) == "plasmas is NULL"
    assert raw(T, a, beam_plasma=None) == "beam_plasma is NULL"
    assert raw(T, a, n_plasmas=0) == "n_plasmas must be 1..4096"
    cfg = T._lib.TraceCfg(0.0, 0, 1e-4, 10, 1, 1.0, 1e-6, 1, 0, 0, 1, s_max=1.0)
    assert raw(T, a, cfg=cfg) == \
        "integrator must be 0 in a multi-beam launch (the adaptive integrator traces one beam per call)"
    cfg = T._lib.TraceCfg(0.0, 0, 1e-4, 10, 1, 1.0, 1e-6, 2, 0)
    assert raw(T, a, cfg=cfg) == \
        "absorption must be 0 or 1 in a multi-beam launch (the warm models trace one beam per call)"


def test_ray_entry_rejections(T, plasmas):
    (a, b, c), far = plasmas
    x, N = rays(5)
    base = dict(beam_off=[0, 3, 5], omega=[OM, OM], mode=[1, -1], plasmas=[a, b, c], beam_plasma=[0, 2])
    for kw, text in ((dict(plasmas=[]), "n_plasmas must be 1..4096"),
                     (dict(plasmas=[a, None, c]), "plasmas[1] is NULL"),
                     (dict(beam_plasma=[0, 3]), "beam_plasma[1] = 3 is outside 0..2 (n_plasmas = 3)"),
                     (dict(beam_plasma=[-1, 0]), "beam_plasma[0] = -1 is outside 0..2 (n_plasmas = 3)"),
                     (dict(plasmas=[far, b, c]),
                      "plasmas[0] is on device 1, the launching handle on device 0 (one device per launch)"),
                     (dict(mode=[1, 2]), "mode[1] must be +1 (X) or -1 (O)")):
        k = dict(base)
        k.update(kw)
        with pytest.raises(T.TorjError) as e:
            T.ray_entry_beams(a, k["beam_off"], k["omega"], k["mode"], x, N, plasmas=k["plasmas"],
                              beam_plasma=k["beam_plasma"])
        assert str(e.value) == text
    L, i, d = T.lib(), T._lib.iptr, T._lib.dptr
    off, om, md = np.array([0, 5], dtype=np.int32), np.array([OM]), np.array([1], dtype=np.int32)
    xs, Ns = (np.ascontiguousarray(v.T) for v in (x, N))
    out = [np.zeros((3, 5)), np.zeros((3, 5)), np.zeros(5), np.zeros(5, dtype=np.int32)]
    for hs, bp, text in ((None, np.zeros(1, dtype=np.int32), "plasmas is NULL"),
                         (T._lib.handles([a]), None, "beam_plasma is NULL")):
        assert L.torj_ray_entry_beams_plasmas_gpu(a.handle, 1, hs, i(bp), 1, i(off), d(om), i(md), d(xs), d(Ns),
                                                  d(out[0]), d(out[1]), d(out[2]), i(out[3])) != 0
        assert L.torj_last_error().decode() == text


def test_wrapper_wants_both_tables(T, plasmas):
    (a, b, _), _ = plasmas
    x, N = rays(5)
    with pytest.raises(ValueError, match="go together"):
        T.trace_beams(a, [0, 5], [OM], [1], x, N, n_steps=10, plasmas=[a, b])
    with pytest.raises(ValueError, match="n_beams entries"):
        T.trace_beams(a, [0, 5], [OM], [1], x, N, n_steps=10, plasmas=[a, b], beam_plasma=[0, 1])


def test_valid_calls_fail_loudly_without_gpu(T, plasmas):
    """No CPU fallback: without a HIP device the valid calls raise."""
    n = ctypes.c_int(0)
    if T.lib().torj_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    (a, b, c), _ = plasmas
    x, N = rays(5)
    with pytest.raises(T.TorjError):
        T.trace_beams(a, [0, 3, 5], [OM, 1.1 * OM], [1, -1], x, N, n_steps=10, absorption=False, plasmas=[b, c],
                      beam_plasma=[1, 0])
    with pytest.raises(T.TorjError):
        T.ray_entry_beams(a, [0, 3, 5], [OM, 1.1 * OM], [1, -1], x, N, plasmas=[b, c], beam_plasma=[1, 0])
