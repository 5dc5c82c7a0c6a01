// torj_split.hpp -- the split RK4 path's host side: the launch plan of one
// call (SplitPlan), the carving of the handle's ring workspace, and the block
// loop with its streams and events (split_trace).
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
//
// The plan's sizes and the carving come first and need no kernel header and no
// HIP call: TORJ_SPLIT_PLAN_ONLY stops the file after them, for a host build
// (tests/native/split_plan_host.hip).
#pragma once
#include <algorithm>
#include <atomic>

#include "torj_args.hpp"
#include "torj_fitdepo.hpp"
#include "torj_host_util.hpp"
#ifndef TORJ_SPLIT_PLAN_ONLY
#include "torj_dispatch.hpp"
#include "torj_k_alpha.hpp"
#include "torj_k_depo.hpp"
#include "torj_k_scan.hpp"
#include "torj_k_traj.hpp"
#include "torj_plasma.hpp"

// dynamic LDS of the walk kernels: the shell grid, when it fits
static size_t fit_grid_lds(int n_psi) { return n_psi <= kFitGridLds ? (size_t)n_psi * sizeof(double) : 0; }

// the reference deposition walk's per-boundary root counts, open-shell spill
// (NaN: every shell closed) and per-ray shell powers, cleared before the walk
// (2 GB on the headline beam: ~0.5 ms)
static int fit_zero(const FitArgs &fa, hipStream_t st) {
    const size_t L = (size_t)fa.n_psi, N = (size_t)fa.n;
    HIPCK(hipMemsetAsync(fa.cnt, 0, (L + 1) * N * sizeof(int), st));
    HIPCK(hipMemsetAsync(fa.Fopen, 0xFF, L * N * sizeof(double), st));
    HIPCK(hipMemsetAsync(fa.dPs, 0, L * N * sizeof(double), st));
    return 0;
}
#endif  // TORJ_SPLIT_PLAN_ONLY

// What one split_trace call launches, fixed before anything is enqueued: the
// blocks, the workspace's byte sizes, and the knobs' values read for this call.
struct SplitPlan {
    static constexpr int R = kSplitRing;
    size_t n;
    int n_steps, nf;
    long kb, first;  // steps per block; the first block's steps (0: uniform blocks)
    int n_blk;
    size_t b_ain, b_alpha, b_awork, b_psib, b_cbx, b_n8, b_n4, b_zf, b_gf, b_dsd, b_dsi, b_defer, b_dcnt, bytes;
    bool zflag_on, gflag_on, dstream, serial;
    int dstream_env, depo_lag, lds_env, tile_cap, nan_step, zflag_nan_from, defer_lrm, zlatch;
    double tile_margin;
    int traj_mode;          // the trajectory kernel of this call (kTrajL2 .. kTrajCell)
    size_t traj_lds_bytes;  // k_traj_lds' dynamic LDS: the whole grid's node table

    int block_k0(int b) const { return (int)(first ? (b == 0 ? 0 : first + (long)(b - 1) * kb) : b * kb); }
    int block_len(int b) const { return (int)std::min<long>(first && b == 0 ? first : kb, n_steps - block_k0(b)); }
    // the steps scanned once block bw's scan has run: the cap of the window behind it
    int window_cap(int bw) const {
        return (int)(first ? (bw == 0 ? first : first + (long)bw * kb) : std::min<long>((long)(bw + 1) * kb, n_steps));
    }
};

// The trajectory kernel TORJ_TRAJ_LDS = lds_env selects on an nR x nZ grid: 3 the
// cell tile, 2 the node tile, 1 the whole-grid table in LDS while it fits 160 KiB
// (lds_bytes: kTrajLdsNS fp64 for each of the (nR + 2)(nZ + 2) coefficients), and
// otherwise -- 1 on a larger grid included -- the L2 kernel
static int split_traj_mode(int lds_env, int nR, int nZ, size_t *lds_bytes) {
    *lds_bytes = (size_t)(nR + 2) * (nZ + 2) * kTrajLdsNS * sizeof(double);
    if (lds_env == 3) return kTrajCell;
    if (lds_env == 2) return kTrajTile;
    return lds_env == 1 && *lds_bytes <= 160 * 1024 ? kTrajLds : kTrajL2;
}

// walk: the reference profile's walk can be streamed behind the scans (fa and dso given);
// negl_skip: the Gauss-Legendre table's early settle is on (GLTable::negl_skip);
// sched_mode, sched_waves: the handle's torj_set_sched; free_b: the device memory free now
static void split_plan_sizes(SplitPlan &pl, int sched_mode, int sched_waves, size_t free_b, const TraceArgs &a,
                             int DM, bool walk, bool negl_skip) {
    const size_t n = pl.n = (size_t)a.n;
    const int n_steps = pl.n_steps = a.n_steps;
    // steps per block: kRing alpha-input buffers within the budget (TORJ_SPLIT_MB
    // per buffer, default 1024: measured 66.5 / 67.8 / 69.4 ms at 1 / 2 / 4 GiB on
    // the headline beam), a multiple of the chunk length
    static const size_t budget_env = (size_t)env_long("TORJ_SPLIT_MB", 1024) << 20;
    // ... and at most 1/16 of the device memory free now for each of the kRing
    // buffers (a quarter of it for the whole ring; 1 GiB on an idle MI355X)
    const size_t budget = std::max<size_t>(std::min(budget_env, free_b / 16), 1);
    pl.nf = a.abs_model >= 2 ? kAinFW : kAinF;
    const size_t per_step = 4 * (size_t)pl.nf * sizeof(double) * n;
    long kb = (long)std::max<size_t>(1, budget / per_step);
    kb = std::min<long>(kb, 16383);  // the alpha kernels' grid.y = 4 kb stays <= 65535
    if (a.chunk_steps > 0 && kb >= a.chunk_steps) kb -= kb % a.chunk_steps;
    if (sched_mode == 3 && sched_waves > 0) kb = std::min(sched_waves, 16383);  // torj_set_sched(p, 3, steps per block)
    kb = pl.kb = std::min<long>(kb, n_steps);
    const int n_cb = (a.chunk_steps > 0 ? n_steps / a.chunk_steps : 0) + 1;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    // work words exist only for a counted launch (a.counters): uncounted
    // (production) launches neither write nor read them, nor reserve them
    pl.b_ain = al(per_step * kb);
    pl.b_alpha = al(4 * sizeof(double) * n * kb);
    pl.b_awork = a.counters ? al(4 * sizeof(unsigned) * n * kb) : 0;
    pl.b_psib = DM == kDepoBinned ? al(sizeof(double) * n * kb) : 0;
    pl.b_cbx = al(6 * sizeof(double) * n * n_cb);
    pl.b_n8 = al(8 * n);
    pl.b_n4 = al(4 * n);
    // the block zero flags (ZBox): Albajar with the early settle on (GLTable::negl_skip);
    // TORJ_ALPHA_ZFLAG=0 (read per call) turns them off
    pl.zflag_on = a.abs_model == 1 && negl_skip && env_int("TORJ_ALPHA_ZFLAG", 1) != 0;
    pl.b_zf = pl.zflag_on ? al(n) : 0;
    // the group flag words, one per 64-ray group and ring slot (SplitArgs::gflag):
    // with the block zero flags unless TORJ_ALPHA_GFLAG=0 (read per call), which
    // restores the per-ray test in k_alpha_pts, its zero stores and the scan's loads.
    // Each slot's array is a multiple of 256 B, so no two slots share a cache line
    pl.gflag_on = pl.zflag_on && env_int("TORJ_ALPHA_GFLAG", 1) != 0;
    pl.b_gf = pl.gflag_on ? al(sizeof(unsigned) * ((n + 63) / 64)) : 0;
    // TORJ_ZBOX_LATCH=0 (read per call): the trajectory kernel keeps growing every
    // ray's box to the end of the block (traj_run's latch; the flags are the same)
    pl.zlatch = env_int("TORJ_ZBOX_LATCH", 1) != 0;
    // the streamed deposition's per-ray walk state (fa: the reference profile;
    // TORJ_DEPO_STREAM=0 runs the whole walk after the trace instead)
    // TORJ_DEPO_STREAM=1: the windows on the scan's stream, after each scan;
    // =2: on a stream of their own, each after its block's scan, so the next
    // scan (and the ring slot it releases) does not wait behind them; =3: on
    // the scan's stream, each window's elimination and walk as two launches
    // (the default since round 4: DESIGN.md 3.4); =4: the two launches on a
    // stream of their own (as 2); =5: see split_trace
    pl.dstream_env = env_int("TORJ_DEPO_STREAM", 3);  // read per call (tests compare both)
    pl.dstream = walk && pl.dstream_env != 0;
    pl.b_dsd = pl.dstream ? al(kDsNd * sizeof(double) * n) : 0;
    pl.b_dsi = pl.dstream ? al(kDsNi * sizeof(int) * n) : 0;
    // TORJ_SPLIT_FIRST: the first block's steps (a multiple of the chunk; 0 =
    // uniform blocks): a short first block lets the alpha kernel start sooner,
    // while the trajectory kernel alone cannot fill the chip
    long first = env_long("TORJ_SPLIT_FIRST", 0);
    if (a.chunk_steps > 0 && first > 0) first = std::max<long>(a.chunk_steps, first - first % a.chunk_steps);
    if (first >= kb || first >= n_steps) first = 0;
    pl.first = first;
    pl.n_blk = first ? 1 + (int)((n_steps - first + kb - 1) / kb) : (int)((n_steps + kb - 1) / kb);
    // warm: the list of deferred (lrm > 3) points of a block (one list: the
    // alpha kernels of consecutive blocks are ordered on one stream) and one
    // counter per block
    pl.b_defer = a.abs_model >= 2 ? al(4 * sizeof(unsigned long long) * n * kb) : 0;
    pl.b_dcnt = a.abs_model >= 2 ? al(sizeof(unsigned) * pl.n_blk) : 0;
    pl.bytes = pl.R * (pl.b_ain + pl.b_alpha + pl.b_awork) + pl.R * pl.b_psib + pl.b_cbx + 6 * pl.b_n8 +
               3 * pl.b_n8 + 2 * pl.b_n4 + pl.b_dsd + pl.b_dsi + pl.b_defer + pl.b_dcnt + pl.R * pl.b_zf + pl.R * pl.b_gf;
    // TORJ_SPLIT_SERIAL=1: every kernel on the caller's stream, no overlap (a
    // measurement aid; read per call so a test can compare both orders)
    pl.serial = env_int("TORJ_SPLIT_SERIAL", 0) != 0;
    pl.depo_lag = std::min(kSplitRing - 1, std::max(1, env_int("TORJ_DEPO_LAG", 2)));
    // the trajectory kernel with the coefficients staged in LDS whenever the grid
    // fits 160 KiB at 6 fp64 per node (56 x 56: 161 KB), one workgroup of wpb
    // waves per CU (measured: trajectory kernel 28.2 -> 24.3 ms, pipeline 67.2 ->
    // 61.6 ms on the headline beam; TORJ_TRAJ_LDS=0 reads them through L2)
    // (read per call: the tests compare the modes; TORJ_TILE_CAP / TORJ_TILE_MARGIN
    // shrink the tile to exercise the global-memory fallback)
    // TORJ_TRAJ_LDS: 3 (default since round 4) the cell-tiled power-form kernel
    // k_traj_cell (trace phase 51.4-51.5 -> 48.9-49.3 ms on the headline beam,
    // alternating); 1 the whole-grid node table in LDS; 2 the node tile; 0 L2
    pl.lds_env = env_int("TORJ_TRAJ_LDS", 3);
    const int tile_max = pl.lds_env == 3 ? kTileCells : kTileNodes;  // cells / nodes
    pl.tile_cap = std::min(tile_max, env_int("TORJ_TILE_CAP", tile_max));
    pl.tile_margin = env_double("TORJ_TILE_MARGIN", 1.001);
    pl.traj_mode = split_traj_mode(pl.lds_env, a.g.nR, a.g.nZ, &pl.traj_lds_bytes);
    // test hook only (tests/test_gpu_split.py): the scan reads alpha as NaN at
    // this step for every third ray -- a stray setting corrupts results, so say so
    pl.nan_step = env_int("TORJ_TEST_NAN_ALPHA_STEP", -1);
    if (pl.nan_step >= 0) {
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true))
            fprintf(stderr, "libtorj_hip: TORJ_TEST_NAN_ALPHA_STEP=%d is set -- a TEST HOOK: alpha is "
                            "read as NaN at that step for every third ray\n", pl.nan_step);
    }
    // test hook only (tests/test_gpu_split.py): TORJ_TEST_ZFLAG_NAN=s -- the fully
    // flagged alpha waves of the blocks that start at step s or later write NaN
    // instead of 0, so that the rays they hold stop NAN where the flags fired
    pl.zflag_nan_from = env_has("TORJ_TEST_ZFLAG_NAN") ? std::max(0, env_int("TORJ_TEST_ZFLAG_NAN", 0)) : -1;
    if (pl.zflag_nan_from >= 0) {
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true))
            fprintf(stderr, "libtorj_hip: TORJ_TEST_ZFLAG_NAN is set -- a TEST HOOK: fully flagged alpha "
                            "waves write NaN\n");
    }
    pl.defer_lrm = std::min(3, std::max(0, env_int("TORJ_WARM_DEFER_LRM", 3)));
}

// SplitArgs::tiny_alpha of a launch: the Gauss-Legendre table's tiny_alpha where the
// trajectory kernel may flag a block by the tiny_alpha bound (tiny_box_flag), else 0.
// Off without the block flags (which need the early settle, negl_skip), in the exact
// leg (tiny_alpha 0), with TORJ_ZBOX_TINY=0 (read per call), and in a counted launch:
// like the h3_fast shortcut, it would move the work counters (a flagged wave counts
// nothing), and bench.py's FLOP model is built on them.
static double split_tiny_alpha(const SplitPlan &pl, const TraceArgs &a, double tiny_alpha) {
    if (!pl.zflag_on || a.counters || !(tiny_alpha > 0.0)) return 0.0;
    return env_int("TORJ_ZBOX_TINY", 1) != 0 ? tiny_alpha : 0.0;
}

// the ring slots and single arrays carved out of the handle's split workspace
struct SplitRing {
    static constexpr int R = SplitPlan::R;
    double *ain[R], *alphas[R], *psib[R];
    unsigned *aworks[R];
    unsigned char *zflags[R];
    unsigned *gflags[R];
    unsigned *dcnt;
    DepoStream ds;
};

// the workspace `q` (pl.bytes) into the ring and sp's per-ray arrays; the
// order fixes every array's alignment, keep it
static void split_carve(const SplitPlan &pl, char *q, SplitArgs &sp, SplitRing &rg) {
    constexpr int R = SplitPlan::R;
    auto take = [&](size_t b) {
        char *r = q;
        q += b;
        return r;
    };
    rg = SplitRing{};
    for (int r = 0; r < R; r++) rg.ain[r] = (double *)take(pl.b_ain);
    for (int r = 0; r < R; r++) {
        rg.alphas[r] = (double *)take(pl.b_alpha);
        rg.aworks[r] = (unsigned *)take(pl.b_awork);
    }
    if (pl.b_psib)
        for (int r = 0; r < R; r++) rg.psib[r] = (double *)take(pl.b_psib);
    if (pl.b_zf)
        for (int r = 0; r < R; r++) rg.zflags[r] = (unsigned char *)take(pl.b_zf);
    if (pl.b_gf)
        for (int r = 0; r < R; r++) rg.gflags[r] = (unsigned *)take(pl.b_gf);
    sp.cbx = (double *)take(pl.b_cbx);
    sp.tx = (double *)take(6 * pl.b_n8);
    sp.stau = (double *)take(pl.b_n8);
    sp.spsi = (double *)take(pl.b_n8);
    sp.sPdep = (double *)take(pl.b_n8);
    sp.tinfo = (int *)take(pl.b_n4);
    sp.sinfo = (int *)take(pl.b_n4);
    sp.defer = pl.b_defer ? (unsigned long long *)take(pl.b_defer) : nullptr;
    rg.dcnt = pl.b_dcnt ? (unsigned *)take(pl.b_dcnt) : nullptr;
    if (pl.dstream) {
        rg.ds.d = (double *)take(pl.b_dsd);
        rg.ds.v = (int *)take(pl.b_dsi);
    }
}

#ifndef TORJ_SPLIT_PLAN_ONLY
static int split_plan(SplitPlan &pl, const torj_plasma_s *p, const TraceArgs &a, int DM, bool walk,
                      bool negl_skip) {
    size_t free_b = 0, total_b = 0;
    HIPCK(hipMemGetInfo(&free_b, &total_b));
    split_plan_sizes(pl, p->sched_mode, p->sched_waves, free_b, a, DM, walk, negl_skip);
    return 0;
}

// The split RK4 path's launches: per block of kb steps, the
// trajectory kernel on the handle's high-priority stream, the alpha and scan
// kernels on its low-priority one, a ring of kRing alpha-input buffers so the
// trajectory runs up to kRing blocks ahead of the alpha; forked from and
// joined back into `s`.
static int split_trace(torj_plasma_s *p, TraceArgs a, int DM, bool tr, hipStream_t s, const FitArgs *fa,
                       DepoStream *dso, bool negl_skip, double tiny_alpha) {
    SplitPlan pl;
    if (split_plan(pl, p, a, DM, fa && dso, negl_skip)) return -1;
    constexpr int R = SplitPlan::R;
    const size_t n = pl.n;
    if (ensure_split(p, pl.bytes)) return -1;
    SplitArgs sp{};
    SplitRing rg;
    split_carve(pl, (char *)p->split.d, sp, rg);
    const DepoStream ds = rg.ds;
    if (dso) *dso = ds;
    sp.nf = pl.nf;
    sp.tile_cap = pl.tile_cap;
    sp.tile_margin = pl.tile_margin;
    sp.nan_step = pl.nan_step;
    sp.zval = 0.0;
    sp.defer_lrm = pl.defer_lrm;
    sp.zlatch = pl.zlatch;
    sp.tiny_alpha = split_tiny_alpha(pl, a, tiny_alpha);
    sp.tval = 0.0;
    // test hook only (tests/test_gpu_tiny_flags.py): TORJ_TEST_TFLAG_NAN=s -- TORJ_TEST_ZFLAG_NAN's
    // twin for the groups flagged by the tiny_alpha proof (word 2): their alphas are NaN in
    // the blocks that start at step s or later.  Two hooks, so that a test can tell which
    // proof flagged a group, and the older hook's tests see the groups they always saw
    const int tflag_nan_from = env_has("TORJ_TEST_TFLAG_NAN") ? std::max(0, env_int("TORJ_TEST_TFLAG_NAN", 0)) : -1;
    if (tflag_nan_from >= 0) {
        static std::atomic<bool> warned{false};
        if (!warned.exchange(true))
            fprintf(stderr, "libtorj_hip: TORJ_TEST_TFLAG_NAN is set -- a TEST HOOK: alpha waves fully "
                            "flagged by the tiny_alpha proof write NaN\n");
    }

    const bool serial = pl.serial, dstream = pl.dstream;
    // the scan on a third stream (TORJ_SPLIT_SCAN=0: behind the alpha kernel on
    // the second), so the alpha kernel of block b + 1 need not wait for the
    // latency-bound one-lane-per-ray scan of block b
    static const bool scan_own = env_int("TORJ_SPLIT_SCAN", 1) != 0;
    hipStream_t sT = serial ? s : p->streamT, s2 = serial ? s : p->stream2;
    hipStream_t s3 = serial ? s : (scan_own ? p->streamS : p->stream2);
    const bool depo_own = dstream && (pl.dstream_env == 2 || pl.dstream_env == 4) && !serial;
    // =5: the windows' two launches on the trajectory kernel's stream, each
    // window `lag` blocks behind its scan (TORJ_DEPO_LAG, default 2, < kRing):
    // the walk's waves then alternate with the trajectory's instead of
    // holding registers beside both it and the alpha kernel
    const bool depo_traj = dstream && pl.dstream_env == 5 && !serial;
    if (depo_own && !p->streamD) {  // created on first use only: one more queue otherwise
        int lo = 0, hi = 0;
        HIPCK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIPCK(hipStreamCreateWithPriority(&p->streamD, hipStreamNonBlocking, stream_prio("TORJ_DEPO_PRIO", lo, lo, hi)));
    }
    hipStream_t sD = depo_own ? p->streamD : s3;
    if (!serial) {  // fork from the caller's stream
        HIPCK(hipEventRecord(p->ev_F, s));
        HIPCK(hipStreamWaitEvent(sT, p->ev_F, 0));
        HIPCK(hipStreamWaitEvent(s2, p->ev_F, 0));
        if (s3 != s2) HIPCK(hipStreamWaitEvent(s3, p->ev_F, 0));
    }
    // the scan's carry starts at (steps 0, OK), tau = 0, P_dep = 0
    HIPCK(hipMemsetAsync(sp.stau, 0, 3 * pl.b_n8, sT));
    HIPCK(hipMemsetAsync(sp.sinfo, 0, pl.b_n4, sT));
    if (dstream) HIPCK(hipMemsetAsync(ds.v + kDsJ * n, 0xFF, n * sizeof(int), sT));  // j = -1: not started
    if (rg.dcnt) HIPCK(hipMemsetAsync(rg.dcnt, 0, pl.n_blk * sizeof(unsigned), s2));  // the alpha kernels' stream
    // the walk's arrays on the scan's stream: the first window runs after the
    // first scan there (or, for TORJ_DEPO_STREAM=2, after an event recorded
    // there), so the clearing overlaps the first trajectory block instead of
    // delaying it (0.5 ms per headline launch)
    if (fa && fit_zero(*fa, s3)) return -1;
    const size_t fit_lds = fa ? fit_grid_lds(fa->n_psi) : 0;
    const int G = (int)((n + 63) / 64);
    const size_t lds_bytes = pl.traj_lds_bytes;
    const bool lds_traj = pl.traj_mode == kTrajLds;
    const bool tile_traj = pl.traj_mode == kTrajTile, cell_traj = pl.traj_mode == kTrajCell;
    sp.traj_mode = pl.traj_mode;
    const int wpb = std::min(8, std::max(1, (G + p->n_cu - 1) / p->n_cu));
    const int n_blocks = pl.n_blk;
    // one window of the streamed walk, its elimination and its walk as two
    // launches, over the steps scanned so far (cap)
    auto depo_pair = [&](hipStream_t st, int cap) {
        hipLaunchKernelGGL(k_depo_elim, dim3(G), dim3(64), 0, st, *fa, ds, sp.sinfo, cap);
        hipLaunchKernelGGL(k_depo_walk, dim3(G), dim3(64), fit_lds, st, *fa, ds, sp.sinfo, cap);
    };
    for (int b = 0; b < n_blocks; b++) {
        sp.k0 = pl.block_k0(b);
        sp.kb = pl.block_len(b);
        const int r = b % R;
        sp.ain = rg.ain[r];
        sp.psib = rg.psib[r];
        sp.zflag = rg.zflags[r];
        sp.gflag = rg.gflags[r];  // null when the group words are off
        sp.zval = (pl.zflag_nan_from >= 0 && sp.k0 >= pl.zflag_nan_from) ? NAN : 0.0;
        sp.tval = (tflag_nan_from >= 0 && sp.k0 >= tflag_nan_from) ? NAN : 0.0;
        sp.alpha = rg.alphas[r];
        sp.awork = pl.b_awork ? rg.aworks[r] : nullptr;  // work words only for a counted launch
        // this ring slot's previous readers (alpha and scan of block b - R) are done
        if (b >= R) HIPCK(hipStreamWaitEvent(sT, p->ev_S[r], 0));
        if (depo_traj && b >= pl.depo_lag) {  // block b - lag's window, behind its scan
            const int bw = b - pl.depo_lag;
            HIPCK(hipStreamWaitEvent(sT, p->ev_S[bw % R], 0));
            depo_pair(sT, pl.window_cap(bw));
        }
        with_depo_traj(DM, tr, [&](auto D, auto T) {
            if (cell_traj)
                hipLaunchKernelGGL((k_traj_cell<D(), T()>), dim3(G), dim3(64), 0, sT, a, sp);
            else if (tile_traj)
                hipLaunchKernelGGL((k_traj_tile<D(), T()>), dim3(G), dim3(64), 0, sT, a, sp);
            else if (lds_traj)
                hipLaunchKernelGGL((k_traj_lds<D(), T()>), dim3(nblocks(G, wpb)), dim3(64 * wpb), lds_bytes, sT, a, sp);
            else
                hipLaunchKernelGGL((k_traj<D(), T()>), dim3(G), dim3(64), 0, sT, a, sp);
        });
        HIPCK(hipEventRecord(p->ev_T[r], sT));
        HIPCK(hipStreamWaitEvent(s2, p->ev_T[r], 0));
        const int nqA = (int)((n + kAlphaBlock - 1) / kAlphaBlock);
        const dim3 agridA((unsigned)nqA, (unsigned)(4 * sp.kb));  // ray groups fastest
        const int nqW = (int)((n + kAlphaWarmBlock - 1) / kAlphaWarmBlock);
        const dim3 agridW((unsigned)nqW, (unsigned)(4 * sp.kb));
        sp.defer_cnt = rg.dcnt ? rg.dcnt + b : nullptr;
#define TORJ_WARM_LAUNCH(IW, C)                                                                     \
    do {                                                                                            \
        hipLaunchKernelGGL((k_alpha_warm_pts<IW, C>), agridW, dim3(kAlphaWarmBlock), 0, s2, a, sp, nqW); \
        hipLaunchKernelGGL((k_alpha_warm_big<IW, C>), dim3(TORJ_WARM_BIG_GRID), dim3(64), 0, s2, a, sp); \
    } while (0)
        if (a.abs_model == 3) {
            if (sp.awork) TORJ_WARM_LAUNCH(3, true);
            else TORJ_WARM_LAUNCH(3, false);
        } else if (a.abs_model == 2) {
            if (sp.awork) TORJ_WARM_LAUNCH(1, true);
            else TORJ_WARM_LAUNCH(1, false);
        }
#undef TORJ_WARM_LAUNCH
#if TORJ_ALPHA_PPW > 1
        else {
            const dim3 agridP((unsigned)nqA, (unsigned)((4 * sp.kb + TORJ_ALPHA_PPW - 1) / TORJ_ALPHA_PPW));
            if (sp.awork)
                hipLaunchKernelGGL((k_alpha_pts_mp<true, TORJ_ALPHA_PPW>), agridP, dim3(kAlphaBlock), 0, s2, a, sp, nqA);
            else
                hipLaunchKernelGGL((k_alpha_pts_mp<false, TORJ_ALPHA_PPW>), agridP, dim3(kAlphaBlock), 0, s2, a, sp, nqA);
        }
#else
        else if (sp.awork)  // a counted launch
            hipLaunchKernelGGL(k_alpha_pts<true>, agridA, dim3(kAlphaBlock), 0, s2, a, sp, nqA);
        else
            hipLaunchKernelGGL(k_alpha_pts<false>, agridA, dim3(kAlphaBlock), 0, s2, a, sp, nqA);
#endif
        HIPCK(hipEventRecord(p->ev_A[r], s2));
        if (s3 != s2) HIPCK(hipStreamWaitEvent(s3, p->ev_A[r], 0));
        with_depo_traj(DM, tr, [&](auto D, auto T) {
            if (a.counters)
                hipLaunchKernelGGL((k_tau_scan_counted<D(), T()>), dim3(G), dim3(64), 0, s3, a, sp);
            else
                hipLaunchKernelGGL((k_tau_scan<D(), T()>), dim3(G), dim3(64), 0, s3, a, sp);
        });
        HIPCK(hipEventRecord(p->ev_S[r], s3));
        // the deposition walk's windows behind this scan (same stream: after it,
        // and the next scan after them; the ring slot is already released)
        // (measured on the headline beam: after every block on the scan's stream
        // 3.62-3.63e9 ray-steps/s; every 2nd / 4th block 3.45-3.64 / 3.58-3.59e9;
        // behind the alpha or the trajectory kernel's stream 3.03 / 2.98e9)
        if (dstream && !depo_traj && b + 1 < n_blocks) {
            if (depo_own) HIPCK(hipStreamWaitEvent(sD, p->ev_S[r], 0));
            if (pl.dstream_env == 3 || pl.dstream_env == 4) {  // elimination and walk as two launches
                // each pair advances a ray by at most one window of kDepoQ
                // segments, so a block of more steps than that takes as many pairs
                // as it has windows (blocks of 120 steps: two), and the walk keeps
                // up with the scan instead of leaving windows for k_depo_tail
                for (int w = 0; w < (sp.kb + kDepoQ - 1) / kDepoQ; w++) depo_pair(sD, sp.k0 + sp.kb);
            } else {
                hipLaunchKernelGGL(k_depo_stream, dim3(G), dim3(64), fit_lds, sD, *fa, ds, sp.sinfo,
                                   sp.k0 + sp.kb);
            }
        }
    }
    if (depo_traj) {  // the last blocks' windows (every block's but the last, as above)
        for (int bw = std::max(0, n_blocks - pl.depo_lag); bw + 1 < n_blocks; bw++) {
            HIPCK(hipStreamWaitEvent(sT, p->ev_S[bw % R], 0));
            depo_pair(sT, pl.window_cap(bw));
        }
    }
    with_depo_traj(DM, tr, [&](auto D, auto T) {
        hipLaunchKernelGGL((k_split_final<D(), T()>), dim3(G), dim3(64), 0, s3, a, sp);
    });
    if (!serial) {  // join: the final kernel followed every scan, each scan its alpha kernel
                    // and each alpha kernel its trajectory
        HIPCK(hipEventRecord(p->ev_J, s3));
        HIPCK(hipStreamWaitEvent(s, p->ev_J, 0));
        if (depo_own || depo_traj) {
            HIPCK(hipEventRecord(p->ev_D, depo_traj ? sT : sD));
            HIPCK(hipStreamWaitEvent(s, p->ev_D, 0));
        }
    }
    HIPCK(hipGetLastError());
    return 0;
}
#endif  // TORJ_SPLIT_PLAN_ONLY
