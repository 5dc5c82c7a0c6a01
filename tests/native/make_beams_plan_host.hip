// Host build of torj_make_beams' compaction (torj.jl_amd/csrc/torj_launch.hpp with
// TORJ_LAUNCH_PLAN_ONLY: no kernel, no HIP call): beams_compact's offsets, gather
// index and per-beam tallies from hand-made entry statuses, pinned without a GPU.
// Test harness only (tests/test_make_beams_plan.py).
#include <hip/hip_runtime.h>

#include "torj_math.hpp"

using namespace torj;

#define TORJ_LAUNCH_PLAN_ONLY 1
#include "torj_launch.hpp"

extern "C" {
// off_c: n_beams + 1; gather: beam_off[n_beams] entries, the first off_c[n_beams] written;
// n_ok, first_bad_ray, first_bad_status: n_beams each.  Returns the number of kept rays.
int mb_compact(int n_beams, const int *beam_off, const int *status, int *off_c, int *gather, int *n_ok,
               int *first_bad_ray, int *first_bad_status) {
    BeamsCompact bc;
    beams_compact(bc, n_beams, beam_off, status);
    if ((int)bc.beam_off.size() != n_beams + 1 || (int)bc.n_ok.size() != n_beams ||
        (int)bc.first_bad_ray.size() != n_beams || (int)bc.first_bad_status.size() != n_beams ||
        (int)bc.gather.size() != bc.beam_off[n_beams] || bc.beam_off[n_beams] > beam_off[n_beams])
        return -1;
    std::copy(bc.beam_off.begin(), bc.beam_off.end(), off_c);
    std::copy(bc.gather.begin(), bc.gather.end(), gather);
    std::copy(bc.n_ok.begin(), bc.n_ok.end(), n_ok);
    std::copy(bc.first_bad_ray.begin(), bc.first_bad_ray.end(), first_bad_ray);
    std::copy(bc.first_bad_status.begin(), bc.first_bad_status.end(), first_bad_status);
    return (int)bc.gather.size();
}
}
