// Host build of the split pipeline's launch plan and workspace carving
// (torj.jl_amd/csrc/torj_split.hpp with TORJ_SPLIT_PLAN_ONLY: no kernel, no HIP
// call): split_plan_sizes' byte counts and split_carve's pointers, the group
// flag words' among them.  The environment knobs are read by the plan itself,
// per call, as in the library.  Test harness only (tests/test_split_plan_gflag.py).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "torj_math.hpp"

using namespace torj;

#define TORJ_SPLIT_PLAN_ONLY 1
#include "torj_split.hpp"

extern "C" {
// n rays, n_steps, chunk_steps, absorption model, counted launch, deposition mode
// (kDepoNone / kDepoBinned / kDepoSamples), the streamed walk, the early settle,
// torj_set_sched's pair and the device's free bytes -> the plan carved at `base`.
// out: bytes, b_gf, b_zf, zflag_on, gflag_on, kRing, kb, n_blk, then the kRing
// zflag pointers and the kRing gflag pointers (0: null), then the first byte
// past the last array carved
int spl_plan(long long n, int n_steps, int chunk_steps, int abs_model, int counted, int depo, int walk,
             int negl_skip, int sched_mode, int sched_waves, unsigned long long free_b, unsigned long long base,
             unsigned long long *out) {
    TraceArgs a{};
    a.n = (int)n;
    a.n_steps = n_steps;
    a.chunk_steps = chunk_steps;
    a.abs_model = abs_model;
    a.counters = counted ? (unsigned long long *)(uintptr_t)8 : nullptr;  // looked at as a flag only
    SplitPlan pl;
    split_plan_sizes(pl, sched_mode, sched_waves, (size_t)free_b, a, depo, walk != 0, negl_skip != 0);
    SplitArgs sp{};
    SplitRing rg;
    split_carve(pl, (char *)(uintptr_t)base, sp, rg);
    int k = 0;
    out[k++] = pl.bytes, out[k++] = pl.b_gf, out[k++] = pl.b_zf, out[k++] = pl.zflag_on, out[k++] = pl.gflag_on;
    out[k++] = SplitPlan::R, out[k++] = (unsigned long long)pl.kb, out[k++] = (unsigned long long)pl.n_blk;
    for (int r = 0; r < SplitPlan::R; r++) out[k++] = (unsigned long long)(uintptr_t)rg.zflags[r];
    for (int r = 0; r < SplitPlan::R; r++) out[k++] = (unsigned long long)(uintptr_t)rg.gflags[r];
    // the last array carved: the streamed walk's integers, else the deferred count, else sinfo
    const char *end = pl.dstream ? (const char *)rg.ds.v + pl.b_dsi
                      : rg.dcnt  ? (const char *)rg.dcnt + pl.b_dcnt
                      : sp.defer ? (const char *)sp.defer + pl.b_defer
                                 : (const char *)sp.sinfo + pl.b_n4;
    out[k++] = (unsigned long long)(uintptr_t)end;
    return k;
}

// the trajectory kernel the plan of an n-ray Albajar call picks on an nR x nZ grid
// under the environment's TORJ_TRAJ_LDS (kTrajL2 .. kTrajCell), and k_traj_lds'
// dynamic LDS bytes for that grid
int spl_traj_mode(long long n, int nR, int nZ, unsigned long long *lds_bytes) {
    TraceArgs a{};
    a.n = (int)n;
    a.n_steps = 6000;
    a.chunk_steps = 60;
    a.abs_model = 1;
    a.g.nR = nR;
    a.g.nZ = nZ;
    SplitPlan pl;
    split_plan_sizes(pl, 3, 60, (size_t)64 << 30, a, kDepoSamples, true, true);
    *lds_bytes = pl.traj_lds_bytes;
    return pl.traj_mode;
}
}
