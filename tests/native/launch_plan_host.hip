// Host build of the library's launch planning (torj.jl_amd/csrc/torj_launch.hpp
// with TORJ_LAUNCH_PLAN_ONLY: no kernel, no HIP call): launch_plan, fit_layout,
// fit_bytes_per_ray and batch_rays, so that the path thresholds and the
// workspace layout are pinned without a GPU.
// Test harness only (tests/test_launch_plan.py).
#include <hip/hip_runtime.h>

#include "torj_math.hpp"

using namespace torj;

#define TORJ_LAUNCH_PLAN_ONLY 1
#include "torj_launch.hpp"

extern "C" {
// has: bit 0 rays (x0, N0, state, status, steps), 1 grid, 2 dP, 3 x_launch, 4 s0, 5 traj;
// knobs: n_cu, sched_mode, sched_waves, lanes_per_ray, TORJ_SCHED, TORJ_SPLIT,
// TORJ_SPLIT_WARM, TORJ_SCHED_W, TORJ_LPR.
// out: path, depo, fit, tr, adaptive, DM, n_save, G, cs, W, S, ctl_bytes, lds,
// hist_off, n_hist, grid, the layout's total bytes
int lp_plan(const torj_trace_cfg *cfg, int n, int n_psi, int has, const int *knobs, long long *out) {
    const LaunchPtrs hp = {(has & 1) != 0, (has & 2) != 0, (has & 4) != 0, (has & 8) != 0, (has & 16) != 0, (has & 32) != 0};
    const LaunchKnobs kn = {knobs[0], knobs[1], knobs[2], knobs[3], knobs[4], knobs[5], knobs[6], knobs[7], knobs[8]};
    LaunchPlan pl;
    if (launch_plan(pl, *cfg, n, n_psi, hp, kn)) return -1;
    const long long v[17] = {pl.path, pl.depo, pl.fit, pl.tr, pl.adaptive, pl.DM, pl.n_save, pl.G, pl.cs, pl.W,
                             (long long)pl.S, (long long)pl.ctl_bytes, (long long)pl.lds, pl.hist_off, pl.n_hist,
                             pl.grid, pl.fit ? (long long)pl.lay.bytes() : 0};
    std::copy(v, v + 17, out);
    return 0;
}
const char *lp_error(void) { return g_err.c_str(); }
// kPathSplit, kPathQueue, kPathLane1, kPathLane16, kTsLds, kSplitMaxSteps
void lp_consts(int *out) {
    const int v[6] = {kPathSplit, kPathQueue, kPathLane1, kPathLane16, kTsLds, kSplitMaxSteps};
    std::copy(v, v + 6, out);
}
// byte offsets of smp_psi, smp_dpds, smp_s, E, Gpsi, GP, cnt, Fopen, dPs, kstar, and the total
void lp_fit_layout(long long n, long long rows, long long n_psi, int store_s, long long *off) {
    const FitLayout l = fit_layout((size_t)n, (size_t)rows, (size_t)n_psi, store_s != 0);
    for (int k = 0; k <= kFaN; k++) off[k] = (long long)l.off[k];
}
long long lp_fit_bytes_per_ray(long long rows, long long n_psi, int store_s) {
    return (long long)fit_bytes_per_ray((size_t)rows, (size_t)n_psi, store_s != 0);
}
long long lp_batch_rays(long long n, long long per_ray, long long budget, long sb_rays) {
    return (long long)batch_rays((size_t)n, (size_t)per_ray, (size_t)budget, sb_rays);
}
}
