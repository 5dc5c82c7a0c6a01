// Host build of the multi-beam launch's planning (torj.jl_amd/csrc/torj_launch.hpp
// with TORJ_LAUNCH_PLAN_ONLY: no kernel, no HIP call): beams_plan's argument
// checks, its choice of lanes per ray and its wave table, pinned without a GPU.
// Test harness only (tests/test_beams_plan.py).
#include <hip/hip_runtime.h>

#include "torj_math.hpp"

using namespace torj;

#define TORJ_LAUNCH_PLAN_ONLY 1
#include "torj_launch.hpp"

extern "C" {
// has and knobs as launch_plan_host.hip's lp_plan.
// out: lanes per ray, waves, rays, depo, fit, tr, DM, n_save, the layout's total bytes;
// waves (beam, first ray) and beams (lo, hi, mode) up to the given capacities
int bp_plan(const torj_trace_cfg *cfg, int n_beams, const int *beam_off, const double *omega, const int *mode,
            int n_psi, int has, const int *knobs, long long *out, int *waves, int waves_cap, int *beams,
            double *beam_omega, int beams_cap) {
    const LaunchPtrs hp = {(has & 1) != 0, (has & 2) != 0, (has & 4) != 0, (has & 8) != 0, (has & 16) != 0, (has & 32) != 0};
    const LaunchKnobs kn = {knobs[0], knobs[1], knobs[2], knobs[3], knobs[4], knobs[5], knobs[6], knobs[7], knobs[8]};
    BeamsPlan bp;
    if (beams_plan(bp, *cfg, n_beams, beam_off, omega, mode, n_psi, hp, kn)) return -1;
    const long long v[9] = {bp.lpr, (long long)bp.waves.size(), bp.n, bp.depo, bp.fit, bp.tr, bp.DM, bp.n_save,
                            bp.fit ? (long long)bp.lay.bytes() : 0};
    std::copy(v, v + 9, out);
    for (size_t w = 0; w < bp.waves.size() && (int)w < waves_cap; w++)
        waves[2 * w] = bp.waves[w].beam, waves[2 * w + 1] = bp.waves[w].first;
    for (size_t b = 0; b < bp.beams.size() && (int)b < beams_cap; b++) {
        beams[3 * b] = bp.beams[b].lo, beams[3 * b + 1] = bp.beams[b].hi, beams[3 * b + 2] = bp.beams[b].mode;
        beam_omega[b] = bp.beams[b].omega;
    }
    return 0;
}
const char *bp_error(void) { return g_err.c_str(); }
int bp_max_beams(void) { return kMaxBeams; }
}
