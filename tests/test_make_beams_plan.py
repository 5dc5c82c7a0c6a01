"""torj_make_beams' compaction (csrc/torj_launch.hpp beams_compact), host build, on
CPU: from the launched beam_off and hand-made entry statuses, the compacted
offsets, the gather index of the rays that entered (launched order within each
beam) and each beam's tally and first failure.  Every expected value is written
out by hand from the statuses."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, REFLECTED, ENTRY_FAIL = 0, 4, 5


@pytest.fixture(scope="module")
def H():
    nat = os.path.join(HERE, "native")
    out = os.path.join(nat, "build", "libmake_beams_plan_host.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    # libbeams_plan_host.so's flags (tests/test_beams_plan.py), host code only
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17", "-fPIC",
                           "-shared", "--offload-arch=gfx950", "--offload-host-only",
                           "-I" + os.path.join(ROOT, "torj.jl_amd", "csrc"), "-o", out,
                           os.path.join(nat, "make_beams_plan_host.hip")])
    L = C.CDLL(out)
    L.mb_compact.argtypes = [C.c_int] + [C.POINTER(C.c_int)] * 7
    return L


def compact(H, counts, status):
    """-> (compacted beam_off, gather, n_ok, first_bad_ray, first_bad_status)"""
    B = len(counts)
    off = [0]
    for c in counts:
        off.append(off[-1] + c)
    n = off[-1]
    assert len(status) == n
    ia = lambda v: (C.c_int * max(len(v), 1))(*v)
    off_c, gather = ia([-7] * (B + 1)), ia([-7] * n)
    n_ok, bad, bad_st = ia([-7] * B), ia([-7] * B), ia([-7] * B)
    m = H.mb_compact(B, ia(off), ia(status), off_c, gather, n_ok, bad, bad_st)
    assert m >= 0
    assert off_c[B] == m
    return list(off_c)[:B + 1], list(gather)[:m], list(n_ok)[:B], list(bad)[:B], list(bad_st)[:B]


def test_all_ok_is_identity(H):
    off, gather, n_ok, bad, bad_st = compact(H, (46, 5, 1), [OK] * 52)
    assert off == [0, 46, 51, 52]
    assert gather == list(range(52))
    assert n_ok == [46, 5, 1]
    assert bad == [-1, -1, -1] and bad_st == [0, 0, 0]


def test_failures_at_start_middle_end(H):
    """three beams of 5: the first's rays 0 and 1 fail, the second's ray 2, the third's ray 4"""
    st = [ENTRY_FAIL, REFLECTED, OK, OK, OK,
          OK, OK, REFLECTED, OK, OK,
          OK, OK, OK, OK, ENTRY_FAIL]
    off, gather, n_ok, bad, bad_st = compact(H, (5, 5, 5), st)
    assert off == [0, 3, 7, 11]
    assert gather == [2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13]
    assert n_ok == [3, 4, 4]
    assert bad == [0, 2, 4]  # within the beam
    assert bad_st == [ENTRY_FAIL, REFLECTED, ENTRY_FAIL]


def test_first_failure_is_the_first(H):
    """several failures in a beam: the first one's index and status are reported, and the
    kept rays keep their launched order"""
    st = [OK, REFLECTED, OK, ENTRY_FAIL, OK, ENTRY_FAIL, OK]
    off, gather, n_ok, bad, bad_st = compact(H, (7,), st)
    assert off == [0, 4] and gather == [0, 2, 4, 6] and n_ok == [4]
    assert (bad, bad_st) == ([1], [REFLECTED])
    st = [OK, ENTRY_FAIL, OK, REFLECTED, OK, ENTRY_FAIL, OK]
    assert compact(H, (7,), st)[3:] == ([1], [ENTRY_FAIL])


def test_whole_beam_failed(H):
    """the middle beam loses every ray: an empty beam between two whole ones"""
    st = [OK] * 4 + [ENTRY_FAIL] * 3 + [OK] * 2
    off, gather, n_ok, bad, bad_st = compact(H, (4, 3, 2), st)
    assert off == [0, 4, 4, 6]
    assert gather == [0, 1, 2, 3, 7, 8]
    assert n_ok == [4, 0, 2]
    assert bad == [-1, 0, -1] and bad_st == [0, ENTRY_FAIL, 0]
    # every beam failed: nothing is kept
    off, gather, n_ok, bad, bad_st = compact(H, (2, 1), [REFLECTED, ENTRY_FAIL, ENTRY_FAIL])
    assert off == [0, 0, 0] and gather == [] and n_ok == [0, 0]
    assert bad == [0, 0] and bad_st == [REFLECTED, ENTRY_FAIL]


def test_empty_launched_beam(H):
    """a launched beam without rays stays empty and reports no failure, wherever it stands"""
    st = [OK, REFLECTED, OK]
    off, gather, n_ok, bad, bad_st = compact(H, (0, 3, 0, 0), st)
    assert off == [0, 0, 2, 2, 2]
    assert gather == [0, 2]
    assert n_ok == [0, 2, 0, 0]
    assert bad == [-1, 1, -1, -1] and bad_st == [0, REFLECTED, 0, 0]


def test_other_nonzero_status_counts_as_failed(H):
    """only status 0 enters (the entry gives 0, 4 or 5; any other value is not kept either)"""
    off, gather, n_ok, bad, bad_st = compact(H, (3,), [OK, 3, OK])
    assert off == [0, 2] and gather == [0, 2] and (bad, bad_st) == ([1], [3])
