// torj_launch.hpp -- one launch of the hot path, planned before it is enqueued
// (the SplitPlan pattern of torj_split.hpp, one level up): launch_plan checks a
// call's arguments and picks its path from them and the knobs alone (LaunchPlan,
// no HIP call, no environment read: tests/test_launch_plan.py pins the
// thresholds on the CPU); fit_layout is the reference deposition's workspace,
// written once for the trace, torj_power_deposition_profile and the batch size;
// trace_device_one enqueues what the plan says, one short launcher per path;
// trace_batched is trace_device's loop over ray batches; beams_plan and
// beams_trace_device are the same two steps for a multi-beam launch, and
// beams_plasmas_plan adds a plasma per beam to that plan; beams_compact closes up the
// rays that passed the ray entry (torj_make_beams).  trace_prologue is what
// both enqueue ahead of their trace kernels, on_caller_stream the NULL stream's
// fork and join around either; a call's arrays reach all of them as one RayIO.
// Also here, ahead of its first user: the Gauss-Legendre table's upload.
// The planning comes first and needs no kernel header: TORJ_LAUNCH_PLAN_ONLY
// stops there (the CPU test's harness).
// (a slice of torj_hip.hip: included after `using namespace torj`)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/torj_hip.h"
#include "torj_args.hpp"
#include "torj_fitdepo.hpp"
#include "torj_host_util.hpp"

// ---- FitLayout: the reference deposition's workspace.  Samples (psi, dP/ds, and
// s where the integrator stores it: RK4 has s0 + k ds) and the elimination's
// coefficients per step, root counts per boundary, open-root integrals and powers
// per shell, the break shell; in this order ----
enum FitArr { kFaPsi, kFaDpds, kFaS, kFaE, kFaGpsi, kFaGP, kFaCnt, kFaFopen, kFaDPs, kFaKstar, kFaN };

// array k's bytes per ray
static size_t fit_arr_bytes(int k, size_t rows, size_t n_psi, bool store_s) {
    if (k <= kFaGP) return k == kFaS && !store_s ? 0 : sizeof(double) * rows;
    return k == kFaCnt ? sizeof(int) * (n_psi + 1) : k == kFaKstar ? sizeof(int) : sizeof(double) * n_psi;
}

// bytes per ray of the layout without its padding: what the batch size is taken from
static size_t fit_bytes_per_ray(size_t rows, size_t n_psi, bool store_s) {
    size_t b = 0;
    for (int k = 0; k < kFaN; k++) b += fit_arr_bytes(k, rows, n_psi, store_s);
    return b;
}

struct FitLayout {
    size_t rows;
    bool store_s;
    size_t off[kFaN + 1];  // byte offsets; off[kFaN]: the total
    size_t bytes() const { return off[kFaN]; }
};

static FitLayout fit_layout(size_t n, size_t rows, size_t n_psi, bool store_s) {
    FitLayout l{rows, store_s, {0}};
    for (int k = 0; k < kFaN; k++) {
        // per-step arrays hold whole 64-ray blocks (smp_at), the int arrays whole 256 bytes
        size_t b = fit_arr_bytes(k, rows, n_psi, store_s) * (k <= kFaGP ? smp_elems(n, 1) : n);
        if (k == kFaCnt || k == kFaKstar) b = (b + 255) & ~(size_t)255;
        l.off[k + 1] = l.off[k] + b;
    }
    return l;
}

// fa's (and a trace's sample) arrays into the workspace at `base`
static void fit_point(const FitLayout &l, char *base, FitArgs &fa, TraceArgs *a) {
    auto D = [&](int k) { return (double *)(base + l.off[k]); };
    double *const smp_s = l.store_s ? D(kFaS) : nullptr;
    fa.rows = l.rows;
    fa.smp_psi = D(kFaPsi), fa.smp_dpds = D(kFaDpds), fa.smp_s = smp_s;
    fa.E = D(kFaE), fa.Gpsi = D(kFaGpsi), fa.GP = D(kFaGP);
    fa.Fopen = D(kFaFopen), fa.dPs = D(kFaDPs);
    fa.cnt = (int *)(base + l.off[kFaCnt]), fa.kstar = (int *)(base + l.off[kFaKstar]);
    if (a) a->smp_psi = D(kFaPsi), a->smp_dpds = D(kFaDpds), a->smp_s = smp_s, a->smp_rows = l.rows;
}

// ---- LaunchPlan: what one trace_device_one call launches, fixed before anything is enqueued ----
// everything the decision reads apart from the call's arguments
struct LaunchKnobs {
    int n_cu, sched_mode, sched_waves, lanes_per_ray;  // the handle's (torj_set_sched)
    // TORJ_SCHED, TORJ_SPLIT, TORJ_SPLIT_WARM (-1 auto, 0 off, 1 on), TORJ_SCHED_W, TORJ_LPR
    int sched_env, split_env, split_warm_env, w_env, lpr_env;
};
// which of the call's pointers are given (rays: x0, N0, state, status and steps, all of them)
struct LaunchPtrs {
    bool rays, grid, dP, x_launch, s0, traj;
};
enum LaunchPath { kPathSplit, kPathQueue, kPathLane1, kPathLane16 };

struct LaunchPlan {
    bool depo, fit, tr, adaptive;
    int DM, n_save;
    LaunchPath path;
    int G, cs;  // 64-ray groups; the queue's steps per visit
    // the queue: W persistent waves, S ring slots, the control block's and the ring's bytes, the
    // dynamic LDS, and in it the binned shells' per-wave histogram (offset and shells, in doubles)
    int W;
    unsigned S;
    size_t ctl_bytes, lds;
    int hist_off, n_hist;
    int grid;       // the one-shot kernels' workgroups
    FitLayout lay;  // fit only
};

static int launch_plan(LaunchPlan &pl, const torj_trace_cfg &cfg, int n, int n_psi, const LaunchPtrs &has,
                       const LaunchKnobs &kn) {
    if (!has.rays) return fail("x0, N0, state, status, steps required");
    if (cfg.n_steps < 0) return fail("n_steps < 0");
    if (cfg.mode != 1 && cfg.mode != -1) return fail("mode must be +1 (X) or -1 (O)");
    if (!(cfg.ds > 0)) return fail("ds must be > 0");
    if (cfg.deposition != 0 && cfg.deposition != 1) return fail("deposition must be 0 or 1");
    if (cfg.integrator != 0 && cfg.integrator != 1) return fail("integrator must be 0 or 1");
    if (cfg.integrator == 1 && (!(cfg.s_max > 0) || cfg.n_chunks < 1 || !(cfg.abstol > 0) ||
                                !(cfg.reltol > 0) || cfg.n_steps < 1))
        return fail("integrator 1 needs s_max > 0, n_chunks >= 1, abstol, reltol > 0, n_steps >= 1");
    pl = LaunchPlan{};
    pl.depo = n_psi >= 2 && has.grid && has.dP;
    pl.fit = pl.depo && cfg.deposition == 1;
    if (pl.fit && (!has.x_launch || !has.s0))
        return fail("deposition = 1 (reference profile) needs x_launch and s0 (torj_trace_ex)");
    if (cfg.absorption < 0 || cfg.absorption > 3) return fail("absorption must be 0..3");
    pl.tr = cfg.traj_stride > 0 && has.traj;
    pl.DM = !pl.depo ? kDepoNone : (pl.fit ? kDepoSamples : kDepoBinned);
    pl.n_save = pl.tr ? cfg.n_steps / cfg.traj_stride : 0;
    const bool adaptive = pl.adaptive = cfg.integrator == 1, warm = cfg.absorption >= 2;
    if (pl.fit) pl.lay = fit_layout((size_t)n, (size_t)cfg.n_steps + 2, (size_t)n_psi, adaptive);
    const int G = pl.G = (n + TORJ_GROUP - 1) / TORJ_GROUP;
    pl.cs = cfg.chunk_steps > 0 ? cfg.chunk_steps : std::max(cfg.n_steps, 1);
    // default: the queue pays off once the beam exceeds one wave per SIMD
    // (measured: 42k rays 111 vs 106 ms one-shot; 100k rays 151 vs 174 ms)
    const bool big = kn.sched_env && G > kn.n_cu * 4;
    // the adaptive path runs one tspan chunk per visit and warm always queues; else
    // any non-zero sched mode is "on": mode 3 sends a cold beam to the queue
    const bool queue = adaptive || warm || (kn.sched_mode >= 0 ? kn.sched_mode != 0 : big);
    // the split RK4 path (fixed steps; sched mode 3 forces it):
    //  * Albajar: by default for beams that would use the work queue;
    //  * warm weakly relativistic (2): by default -- its alpha kernel runs two
    //    waves per SIMD where the fused queue kernel holds one (C5: 165 vs 221 ms);
    //  * warm fully relativistic (3): by default for beams of fewer 64-ray groups
    //    than 3 per CU, where the one-wave-per-SIMD queue kernel leaves SIMDs idle
    //    and the split's alpha kernel spreads the points over all of them (129
    //    rays: 13.1 s -> 0.1 s); on the 1e5-ray fan the queue kernel is faster
    //    (19.7 vs 20.4 s)
    const bool albajar_split = cfg.absorption == 1 && kn.split_env == 1 && big;
    const bool warm_split = warm && kn.split_env == 1 &&
                            (kn.split_warm_env == 1 ||
                             (kn.split_warm_env < 0 && (cfg.absorption == 2 || G < kn.n_cu * 3)));
    // (the split kernels pack a ray's step count into 24 bits beside its status:
    // 0 < n_steps < kSplitMaxSteps, also under mode 3)
    const bool split = !adaptive && cfg.absorption >= 1 && cfg.n_steps > 0 && cfg.n_steps < kSplitMaxSteps &&
                       (kn.sched_mode == 3 || (kn.sched_mode < 0 && (albajar_split || warm_split)));
    if (split) {
        pl.path = kPathSplit;
    } else if (queue && cfg.n_steps > 0) {
        pl.path = kPathQueue;
        // W persistent waves: at most 2 per SIMD (4 SIMDs per CU), and fewer
        // than G so the ready queue keeps a backlog (a wave never waits for a
        // group while another holds it); TORJ_SCHED_W overrides.
        const int W = kn.sched_waves > 0 ? kn.sched_waves
                      : kn.w_env > 0     ? kn.w_env
                                         : std::min(kn.n_cu * 4 * (warm ? TORJ_WARM_MIN_WAVES : TORJ_MIN_WAVES), G - G / 16);
        pl.W = std::max(1, std::min(W, G));
        pl.S = 4u * (unsigned)(G + pl.W);  // ring slots (tag check makes reuse safe)
        pl.ctl_bytes = 256 + (size_t)pl.S * sizeof(unsigned long long);
        // binned shells: a per-wave LDS histogram (RK4, up to 4096 shells; the
        // adaptive path's 25 KB of stage vectors leave no room without losing
        // occupancy, it keeps the global atomics)
        pl.hist_off = adaptive ? kTsLds : 0;
        pl.n_hist = (pl.DM == kDepoBinned && !adaptive && n_psi <= 4096) ? n_psi : 0;
        pl.lds = (size_t)(pl.hist_off + pl.n_hist) * sizeof(double);
    } else {
        // one launch; a beam that would queue comes here with n_steps == 0, the
        // warm models then on the cold instance (launch_lanes).
        // Small Albajar beams: 16 lanes per ray while n x 16 lanes fit two
        // waves per SIMD (the latency of a ray's step chain sets the time there)
        // (TORJ_LPR=1 in the environment turns the automatic choice off)
        const bool lanes16 = cfg.absorption == 1 && pl.DM != kDepoBinned && kn.lanes_per_ray != 1 &&
                             (kn.lanes_per_ray == 16 ||
                              (kn.lpr_env != 1 && (size_t)n * 16 <= (size_t)kn.n_cu * 4 * 2 * 64));
        pl.path = lanes16 ? kPathLane16 : kPathLane1;
        pl.grid = nblocks(lanes16 ? n * 16 : n, TORJ_BLOCK);
    }
    return 0;
}

// rays per launch: all n, or whole 64-ray groups within the workspace budget
// (per_ray: fit_bytes_per_ray, 0 without the reference deposition), and at most
// sb_rays when that is set (TORJ_SPLIT_BATCH)
static size_t batch_rays(size_t n, size_t per_ray, size_t budget, long sb_rays) {
    const size_t nb = per_ray && n * per_ray > budget ? std::max<size_t>(64, budget / per_ray / 64 * 64) : n;
    return sb_rays > 0 && (size_t)sb_rays < nb ? (size_t)sb_rays : nb;
}

// ---- BeamsPlan: a multi-beam launch of the one-shot kernel (torj_trace_beams_device):
// B beams' rays concatenated, beam b rays beam_off[b] .. beam_off[b + 1] - 1 with its
// own omega[b] and mode[b] (cfg.omega, cfg.mode unused) and row b of dP_shell.
// The wave table: beam b takes ceil(n_b / (64 / LPR)) waves, wave j of a beam its rays
// (64 / LPR) j ..., exactly k_trace's lanes on that beam alone -- a wave never mixes
// beams, so the 16-lane Albajar code's per-wave choices see the rays they would in a
// single-beam launch (bit-identical results) and the beam's constants are wave-uniform.
// At most kMaxBeams beams: k_shell_sum_beams' grid is (n_psi, n_beams), its y extent
// limited to 65 535.
constexpr int kMaxBeams = 4096;

struct BeamsPlan {
    bool depo, fit, tr;
    int DM, n_save;
    int n;    // rays of all beams
    int lpr;  // lanes per ray: 1 or 16
    FitLayout lay;  // fit only, for all n rays
    std::vector<BeamRec> beams;
    std::vector<BeamWave> waves;  // the launch's workgroups, one wave each
};

// the three host tables of a multi-beam call, checked (the trace's and the ray entry's)
static int beams_tables_check(int n_beams, const int *beam_off, const double *omega, const int *mode) {
    if (n_beams < 1 || n_beams > kMaxBeams) return fail("n_beams must be 1..%d", kMaxBeams);
    if (!beam_off) return fail("beam_off is NULL");
    if (!omega || !mode) return fail("omega and mode (n_beams each) required");
    if (beam_off[0] != 0) return fail("beam_off[0] must be 0");
    for (int b = 0; b < n_beams; b++)
        if (beam_off[b + 1] < beam_off[b]) return fail("beam_off must not decrease (beam %d)", b);
    for (int b = 0; b < n_beams; b++) {
        if (!(omega[b] > 0) || !std::isfinite(omega[b])) return fail("omega[%d] must be finite and > 0", b);
        if (mode[b] != 1 && mode[b] != -1) return fail("mode[%d] must be +1 (X) or -1 (O)", b);
    }
    return 0;
}
static std::vector<BeamRec> beams_records(int n_beams, const int *beam_off, const double *omega, const int *mode) {
    std::vector<BeamRec> r(n_beams);
    for (int b = 0; b < n_beams; b++)
        r[b] = BeamRec{omega[b], make_consts(omega[b]), mode[b], beam_off[b], beam_off[b + 1]};
    return r;
}

static int beams_plan(BeamsPlan &bp, const torj_trace_cfg &cfg, int n_beams, const int *beam_off,
                      const double *omega, const int *mode, int n_psi, const LaunchPtrs &has,
                      const LaunchKnobs &kn) {
    if (beams_tables_check(n_beams, beam_off, omega, mode)) return -1;
    if (!has.rays) return fail("x0, N0, state, status, steps required");
    if (cfg.n_steps < 0) return fail("n_steps < 0");
    if (!(cfg.ds > 0)) return fail("ds must be > 0");
    if (cfg.deposition != 0 && cfg.deposition != 1) return fail("deposition must be 0 or 1");
    if (cfg.absorption != 0 && cfg.absorption != 1)
        return fail("absorption must be 0 or 1 in a multi-beam launch (the warm models trace one beam per call)");
    if (cfg.integrator != 0)
        return fail("integrator must be 0 in a multi-beam launch (the adaptive integrator traces one beam per call)");
    if (kn.sched_mode == 1 || kn.sched_mode == 3)
        return fail("sched mode %d has no multi-beam form: only the one-shot kernel (torj_set_sched -1, 0, 2)",
                    kn.sched_mode);
    bp = BeamsPlan{};
    bp.depo = n_psi >= 2 && has.grid && has.dP;
    bp.fit = bp.depo && cfg.deposition == 1;
    if (bp.fit && (!has.x_launch || !has.s0))
        return fail("deposition = 1 (reference profile) needs x_launch and s0 (torj_trace_ex)");
    bp.tr = cfg.traj_stride > 0 && has.traj;
    bp.DM = !bp.depo ? kDepoNone : (bp.fit ? kDepoSamples : kDepoBinned);
    bp.n_save = bp.tr ? cfg.n_steps / cfg.traj_stride : 0;
    bp.n = beam_off[n_beams];
    if (bp.fit) bp.lay = fit_layout((size_t)bp.n, (size_t)cfg.n_steps + 2, (size_t)n_psi, false);
    // launch_plan's rule for 16 lanes per ray, on the padded lanes: whole waves per beam
    size_t waves16 = 0;
    for (int b = 0; b < n_beams; b++) waves16 += (size_t)(beam_off[b + 1] - beam_off[b] + 3) / 4;
    const bool lanes16 = cfg.absorption == 1 && bp.DM != kDepoBinned && kn.lanes_per_ray != 1 &&
                         (kn.lanes_per_ray == 16 ||
                          (kn.lpr_env != 1 && waves16 * 64 <= (size_t)kn.n_cu * 4 * 2 * 64));
    bp.lpr = lanes16 ? 16 : 1;
    const int rpw = 64 / bp.lpr;  // rays per wave
    bp.beams = beams_records(n_beams, beam_off, omega, mode);
    for (int b = 0; b < n_beams; b++)
        for (int i = beam_off[b]; i < beam_off[b + 1]; i += rpw) bp.waves.push_back(BeamWave{b, i});
    return 0;
}

// ---- BeamsCompact: the rays of a multi-beam launch that passed the ray entry, closed up
// (torj_make_beams: a ray that fails entry is reported, and the others are traced).  From
// the launched beam_off and the n = beam_off[n_beams] entry statuses (0: entered): the
// compacted beam_off; `gather`, the launched index of compacted ray k, in launched order
// within each beam (stable), so a beam's kept rays sit in the waves they would sit in
// were they launched alone; and per beam its kept count and its first failure (the ray's
// index within the beam and its status; -1 and 0 where every ray entered).  A beam none
// of whose rays entered becomes an empty beam, which beams_plan allows.  No HIP call.
struct BeamsCompact {
    std::vector<int> beam_off;  // n_beams + 1
    std::vector<int> gather;    // beam_off[n_beams]
    std::vector<int> n_ok, first_bad_ray, first_bad_status;  // n_beams each
};

static void beams_compact(BeamsCompact &bc, int n_beams, const int *beam_off, const int *status) {
    bc = BeamsCompact{};
    bc.beam_off.assign(1, 0);
    bc.gather.reserve((size_t)beam_off[n_beams]);
    for (int b = 0; b < n_beams; b++) {
        int bad = -1;
        for (int i = beam_off[b]; i < beam_off[b + 1]; i++) {
            if (status[i] == TORJ_RAY_OK)
                bc.gather.push_back(i);
            else if (bad < 0)
                bad = i;
        }
        bc.beam_off.push_back((int)bc.gather.size());
        bc.n_ok.push_back(bc.beam_off[b + 1] - bc.beam_off[b]);
        bc.first_bad_ray.push_back(bad < 0 ? -1 : bad - beam_off[b]);
        bc.first_bad_status.push_back(bad < 0 ? 0 : status[bad]);
    }
}

// ---- BeamsPlasmasPlan: a multi-beam launch whose beams go through differing plasmas
// (torj_trace_beams_plasmas_device): beam b through the listed plasma beam_plasma[b].
// It is beams_plan's plan -- the wave table, the lanes per ray on the whole launch's
// padded lanes, the workspace of all n rays -- plus the per-beam plasma index and one
// record per listed plasma, in listed order (a plasma may be listed twice or unused).
// The listed handles are opaque here: the caller says how to read one (PlasmaView).
constexpr int kMaxPlasmas = 4096;

struct PlasmaView {
    int (*device)(const void *handle);
    PlasmaRec (*rec)(const void *handle);  // device pointers: valid once the handle's device state exists
};

struct BeamsPlasmasPlan {
    BeamsPlan bp;
    std::vector<int> beam_pl;        // n_beams
    std::vector<PlasmaRec> plasmas;  // n_plasmas
};

// the two host tables the plasma form adds, checked; `device` is the launching handle's
static int beams_plasmas_check(int n_plasmas, const void *const *plasmas, const int *beam_plasma, int device,
                               const PlasmaView &view) {
    if (n_plasmas < 1 || n_plasmas > kMaxPlasmas) return fail("n_plasmas must be 1..%d", kMaxPlasmas);
    if (!plasmas) return fail("plasmas is NULL");
    if (!beam_plasma) return fail("beam_plasma is NULL");
    for (int j = 0; j < n_plasmas; j++)
        if (!plasmas[j]) return fail("plasmas[%d] is NULL", j);
    for (int j = 0; j < n_plasmas; j++)
        if (view.device(plasmas[j]) != device)
            return fail("plasmas[%d] is on device %d, the launching handle on device %d (one device per launch)", j,
                        view.device(plasmas[j]), device);
    return 0;
}
// (after beams_tables_check: n_beams is within its range)
static int beam_plasma_check(int n_plasmas, const int *beam_plasma, int n_beams) {
    for (int b = 0; b < n_beams; b++)
        if (beam_plasma[b] < 0 || beam_plasma[b] >= n_plasmas)
            return fail("beam_plasma[%d] = %d is outside 0..%d (n_plasmas = %d)", b, beam_plasma[b], n_plasmas - 1,
                        n_plasmas);
    return 0;
}

static int beams_plasmas_plan(BeamsPlasmasPlan &pp, const torj_trace_cfg &cfg, int n_plasmas,
                              const void *const *plasmas, const int *beam_plasma, int device, const PlasmaView &view,
                              int n_beams, const int *beam_off, const double *omega, const int *mode, int n_psi,
                              const LaunchPtrs &has, const LaunchKnobs &kn) {
    if (beams_plasmas_check(n_plasmas, plasmas, beam_plasma, device, view)) return -1;
    if (beams_plan(pp.bp, cfg, n_beams, beam_off, omega, mode, n_psi, has, kn)) return -1;
    if (beam_plasma_check(n_plasmas, beam_plasma, n_beams)) return -1;
    pp.beam_pl.assign(beam_plasma, beam_plasma + n_beams);
    pp.plasmas.resize(n_plasmas);
    for (int j = 0; j < n_plasmas; j++) pp.plasmas[j] = view.rec(plasmas[j]);
    return 0;
}

#ifndef TORJ_LAUNCH_PLAN_ONLY
#include <mutex>

#include "torj_dispatch.hpp"
#include "torj_k_beams.hpp"
#include "torj_k_fused.hpp"
#include "torj_k_points.hpp"
#include "torj_split.hpp"

// ---- Gauss-Legendre table (abs_Al_init, src/absorption.jl:1-7): the host copy and
// its upload into c_gl (torj_k_fused.hpp), once per device and version ----
static std::mutex g_gl_mu;
static GLTable g_gl_host;
static int g_gl_version = 0;         // 0: abs_Al_init never called
static int g_gl_uploaded[64] = {0};  // per device

static int ensure_gl_on_device(int dev) {
    std::lock_guard<std::mutex> lk(g_gl_mu);
    if (g_gl_version == 0)
        return fail(
            "The weights and abscissae for the absorption were never initialized. Call "
            "`abs_Al_init` before using the absorption.");
    if (dev < 0 || dev >= 64) return fail("device index %d out of range", dev);
    if (g_gl_uploaded[dev] != g_gl_version) {
        HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(c_gl), &g_gl_host, sizeof(GLTable)));
        g_gl_uploaded[dev] = g_gl_version;
    }
    return 0;
}

// the knobs of a call on handle p; the environment's are read once, at the first trace
static LaunchKnobs launch_knobs(const torj_plasma_s *p) {
    static const int env[5] = {env_int("TORJ_SCHED", 1), env_int("TORJ_SPLIT", 1), env_int("TORJ_SPLIT_WARM", -1),
                               env_int("TORJ_SCHED_W", 0), env_int("TORJ_LPR", 0)};
    return {p->n_cu, p->sched_mode, p->sched_waves, p->lanes_per_ray, env[0], env[1], env[2], env[3], env[4]};
}

// ---- the launchers: one per path, and the phase after the trace ----
// the work-queue kernel (warm models: the TRAJ instance only, with traj_stride
// = 0 when no trajectory is wanted -- fewer instances of the heavy warm code)
static int launch_queue(torj_plasma_s *p, TraceArgs &a, const LaunchPlan &pl, hipStream_t s) {
    if (ensure_buf(p, p->sched, pl.ctl_bytes)) return -1;
    HIPCK(hipMemsetAsync(p->sched.d, 0, pl.ctl_bytes, s));
    SchedCtl *ctl = (SchedCtl *)p->sched.d;
    unsigned long long *slots = (unsigned long long *)((char *)p->sched.d + 256);
    const dim3 grd(pl.W), blk(64);
    a.hist_off = pl.hist_off, a.n_hist = pl.n_hist;
    with_abs_depo_traj(a.abs_model, pl.DM, pl.tr, [&](auto A, auto D, auto Tr) {
        constexpr bool T = A() >= 2 || Tr();
        if (pl.adaptive)
            hipLaunchKernelGGL((k_trace_sched<A(), D(), T, 1>), grd, blk, pl.lds, s, a, ctl, slots, pl.S, pl.G, pl.cs);
        else
            hipLaunchKernelGGL((k_trace_sched<A(), D(), T, 0>), grd, blk, pl.lds, s, a, ctl, slots, pl.S, pl.G, pl.cs);
    });
    // the queue's watchdog / retirement state into the sticky flags
    hipLaunchKernelGGL(k_sched_fold, dim3(1), dim3(1), 0, s, ctl, (unsigned)pl.G, p->d_flags);
    return 0;
}

// k_trace, one lane or 16 per ray.  It exists for the cold model and Albajar only
// (a warm beam gets here with n_steps == 0 alone and takes the cold instance), its
// 16-lane form for Albajar without binned deposition.
static void launch_lanes(const TraceArgs &a, const LaunchPlan &pl, hipStream_t s) {
    const dim3 grd(pl.grid), blk(TORJ_BLOCK);
    if (pl.path == kPathLane16)
        with_depo_traj(pl.DM, pl.tr, [&](auto D, auto T) {
            if constexpr (D() != kDepoBinned) hipLaunchKernelGGL((k_trace<1, D(), T(), 16>), grd, blk, 0, s, a);
        });
    else
        with_abs_depo_traj(a.abs_model == 1 ? 1 : 0, pl.DM, pl.tr, [&](auto A, auto D, auto T) {
            if constexpr (A() <= 1) hipLaunchKernelGGL((k_trace<A(), D(), T()>), grd, blk, 0, s, a);
        });
}

// after a trace with the reference deposition: alpha at the last point, the walk
// (its tail when the split pipeline streamed it: dstr.v) and the shells' sums
static int launch_post(const TraceArgs &a, const FitArgs &fa, const LaunchPlan &pl, const DepoStream &dstr,
                       hipStream_t s) {
    const dim3 grd(nblocks(a.n, 64)), blk(64);
    if (!pl.adaptive)  // (adaptive: the last accepted step's FSAL stage already gave P alpha there)
        with_abs(a.abs_model, [&](auto A) { hipLaunchKernelGGL(k_final_alpha<A()>, grd, blk, 0, s, a); });
    const size_t lds = fit_grid_lds(fa.n_psi);
    if (dstr.v)  // the streamed walk's windows ran behind the scans
        hipLaunchKernelGGL(k_depo_tail, grd, blk, lds, s, fa, dstr);
    else
        hipLaunchKernelGGL(k_fit_depo, grd, blk, lds, s, fa);
    hipLaunchKernelGGL(k_shell_sum, dim3(fa.n_psi), dim3(256), 0, s, fa);
    HIPCK(hipGetLastError());
    return 0;
}

// torj_timing: this call's three events (start, trace end, post end) from the
// handle's pool, the first recorded on `s`; all null when timing is off
static int timing_begin(torj_plasma_s *p, hipEvent_t ev[3], hipStream_t s) {
    ev[0] = ev[1] = ev[2] = nullptr;
    if (!p->timing) return 0;
    while (p->ev_used + 3 > p->ev_pool.size()) {
        hipEvent_t e;
        HIPCK(hipEventCreate(&e));
        p->ev_pool.push_back(e);
    }
    for (int q = 0; q < 3; q++) ev[q] = p->ev_pool[p->ev_used + q];
    p->ev_used += 3;
    HIPCK(hipEventRecord(ev[0], s));
    return 0;
}

// A device-pointer entry's stream: call(s) with the caller's, or, for the NULL (legacy
// default) stream, with the handle's own non-blocking stream, after the NULL stream's
// earlier work and before its later work (the same ordering); enqueued on the NULL
// stream itself the trace phase ran ~0.4 ms slower per headline launch (implicit
// synchronisation with the blocking streams)
template <class F>
static int on_caller_stream(torj_plasma_s *p, void *stream, F call) {
    if (stream) return call((hipStream_t)stream);
    if (ensure_device(p)) return -1;
    if (!p->ev_Nin) {
        HIPCK(hipEventCreateWithFlags(&p->ev_Nin, hipEventDisableTiming));
        HIPCK(hipEventCreateWithFlags(&p->ev_Nout, hipEventDisableTiming));
    }
    HIPCK(hipEventRecord(p->ev_Nin, nullptr));
    HIPCK(hipStreamWaitEvent(p->stream, p->ev_Nin, 0));
    const int rc = call(p->stream);
    HIPCK(hipEventRecord(p->ev_Nout, p->stream));
    HIPCK(hipStreamWaitEvent(nullptr, p->ev_Nout, 0));
    return rc;
}

// ---- RayIO: a trace's ray count and arrays, passed on by every host layer below the extern "C"
// functions (a layer's own arrays: set by name on a copy); n_psi beside it, 0 without deposition ----
using RayIO = torj_beam_shard;
static LaunchPtrs launch_ptrs(const RayIO &io) {  // which of its pointers are given
    return {io.x0 && io.N0 && io.state && io.status && io.steps, io.psi_grid != nullptr, io.dP_shell != nullptr,
            io.x_launch != nullptr, io.s0 != nullptr, io.traj != nullptr};
}
// doubles in n_dP rows of dP_shell: n_psi + 1 each (one where there is no grid)
static size_t dP_rows(int n_dP, int n_psi) { return (size_t)n_dP * (size_t)(n_psi > 0 ? n_psi + 1 : 1); }
// the host tables of a multi-beam call, in the order every entry takes them
struct BeamTables { int n_beams; const int *beam_off; const double *omega; const int *mode; };

// the kernels' arguments that come from the handle, the cfg and the caller's arrays alone
static TraceArgs trace_args(const torj_plasma_s *p, const torj_trace_cfg &cfg, const RayIO &io) {
    TraceArgs a{};
    a.coef = p->d_coef, a.cellp = p->d_cellp, a.g = p->g;
    a.k = make_consts(cfg.omega), a.omega = cfg.omega, a.mode = cfg.mode, a.abs_model = cfg.absorption;
    a.ds = cfg.ds, a.n_steps = cfg.n_steps, a.chunk_steps = cfg.chunk_steps;
    a.psi_exit = cfg.psi_exit, a.P_min = cfg.P_min;
    a.n = io.n, a.x0 = io.x0, a.N0 = io.N0, a.w = io.weights, a.s0 = io.s0;
    a.state = io.state, a.status = io.status, a.steps = io.steps, a.counters = (unsigned long long *)io.counters;
    if (cfg.integrator == 1) {
        a.abstol = cfg.abstol, a.reltol = cfg.reltol;
        a.s_step = cfg.s_max / cfg.n_chunks, a.n_chunks = cfg.n_chunks;
    }
    return a;
}

// the walk's arguments beside its workspace (fit_point), from the trace's
static void fit_args(FitArgs &fa, const TraceArgs &a, const double *x_launch, bool s_uniform) {
    fa.coef = a.coef, fa.g = a.g, fa.n = a.n, fa.n_psi = a.n_psi, fa.ds = a.ds;
    // boundary lookups guess from grid[0], grid[n-1] in-kernel and correct
    // locally: no host read of the (device-resident) grid, no stream sync
    fa.grid = a.grid, fa.w = a.w, fa.x_launch = x_launch, fa.s0 = a.s0, fa.steps = a.steps;
    fa.s_uniform = s_uniform;  // RK4: s_k = s0 + k ds, not stored
    fa.dP = a.dP, fa.Pray = a.Pdep;
}

// What a launch sets up and enqueues ahead of its trace kernels, from either plan
// (LaunchPlan, BeamsPlan: depo, fit, tr, n_save, lay): the deposition's arguments with
// the P_dep workspace, the walk's workspace and arguments, then in `s`'s order
// k_grid_check, the NaN fill of traj, fit_zero and the timing's first event.
// zero = false leaves fit_zero to the caller.
template <class Plan>
static int trace_prologue(torj_plasma_s *p, const Plan &pl, const torj_trace_cfg &cfg, const RayIO &io, int n_psi,
                          bool s_uniform, bool zero, TraceArgs &a, FitArgs &fa, hipEvent_t ev[3], hipStream_t s) {
    if (pl.depo) {
        a.n_psi = n_psi;
        a.grid = io.psi_grid;  // uniform-grid fast path is set up in-kernel from grid[0], grid[n-1]
        a.dP = io.dP_shell, a.Pdep = io.P_dep;
        if (!a.Pdep) {  // the work-queue kernel carries P_dep across chunks: workspace
            if (ensure_buf(p, p->ws, (size_t)a.n * sizeof(double))) return -1;
            a.Pdep = (double *)p->ws.d;
        }
    }
    if (pl.fit) {
        if (ensure_buf(p, p->fit, pl.lay.bytes())) return -1;
        fit_point(pl.lay, (char *)p->fit.d, fa, &a);
        fit_args(fa, a, io.x_launch, s_uniform);
    }
    if (pl.depo)  // psi_dP_dV strictly increasing: checked on the device, reported by torj_trace_check
        hipLaunchKernelGGL(k_grid_check, dim3(1), dim3(256), 0, s, io.psi_grid, n_psi, p->d_flags);
    if (pl.tr) {
        a.traj_stride = cfg.traj_stride, a.n_save = pl.n_save, a.traj = io.traj;
        if (a.n_save > 0)
            HIPCK(hipMemsetAsync(io.traj, 0xFF, (size_t)a.n_save * 5 * a.n * sizeof(double), s));  // NaN
    }
    if (pl.fit && zero && fit_zero(fa, s)) return -1;
    return timing_begin(p, ev, s);
}

// one launch of the hot path over io.n rays
static int trace_device_one(torj_plasma_t p, const torj_trace_cfg *cfg, const RayIO &io, int n_psi, hipStream_t s) {
    const int n = io.n;
    if (n <= 0) return 0;
    const LaunchPtrs has = launch_ptrs(io);
    LaunchPlan pl;
    const bool fresh = !p->d_flags;  // n_cu is the device's only once ensure_device has run
    if (launch_plan(pl, *cfg, n, n_psi, has, launch_knobs(p))) return -1;  // argument errors need no device
    if (ensure_device(p)) return -1;
    if (fresh && launch_plan(pl, *cfg, n, n_psi, has, launch_knobs(p))) return -1;
    if (cfg->absorption == 1 && ensure_gl_on_device(p->device)) return -1;
    TraceArgs a = trace_args(p, *cfg, io);
    if (pl.adaptive) {
        if (ensure_buf(p, p->chunk, (size_t)n * sizeof(int))) return -1;
        a.chunk = (int *)p->chunk.d;
    }
    // the fused / queue paths clear the deposition workspace before the trace
    // phase's first event (outside trace_ms, as before round 5); the split path
    // clears it on its scan stream, overlapped with the first trajectory block
    FitArgs fa{};
    hipEvent_t ev[3];
    if (trace_prologue(p, pl, *cfg, io, n_psi, !pl.adaptive, pl.path != kPathSplit, a, fa, ev, s)) return -1;
    DepoStream dstr{};  // the split pipeline's streamed deposition (split_trace)
    switch (pl.path) {
    case kPathSplit:
        if (split_trace(p, a, pl.DM, pl.tr, s, pl.fit ? &fa : nullptr, &dstr, g_gl_host.negl_skip != 0,
                        g_gl_host.tiny_alpha))
            return -1;
        break;
    case kPathQueue:
        if (launch_queue(p, a, pl, s)) return -1;
        break;
    case kPathLane1:
    case kPathLane16: launch_lanes(a, pl, s);
    }
    HIPCK(hipGetLastError());
    if (ev[1]) HIPCK(hipEventRecord(ev[1], s));
    if (pl.fit && launch_post(a, fa, pl, dstr, s)) return -1;
    if (ev[2]) HIPCK(hipEventRecord(ev[2], s));
    return 0;
}

// ---- a multi-beam launch (torj_trace_beams_device, torj_ray_entry_beams_device) ----
// the plan's tables into the handle's buffer, in `s`'s order: the beams' records, then
// the waves'.  The copy is from pageable memory, which HIP has consumed when the call
// returns; the buffer is the handle's scratch (one stream per handle), so a launch
// enqueued earlier on `s` has read its own tables before these arrive.  `plasmas` and
// `beam_pl` are empty unless the launch goes through several plasmas.
static int beams_upload(torj_plasma_s *p, const std::vector<BeamRec> &beams, const std::vector<BeamWave> &waves,
                        const std::vector<PlasmaRec> &plasmas, const std::vector<int> &beam_pl, hipStream_t s,
                        const BeamRec **d_beams, const BeamWave **d_waves, const PlasmaRec **d_plasmas,
                        const int **d_beam_pl) {
    // (every table's size is a multiple of 8 bytes but the last's, so each starts aligned)
    const size_t nb = beams.size() * sizeof(BeamRec), nw = waves.size() * sizeof(BeamWave);
    const size_t np = plasmas.size() * sizeof(PlasmaRec), ni = beam_pl.size() * sizeof(int);
    if (ensure_buf(p, p->beams, nb + nw + np + ni)) return -1;
    char *d = (char *)p->beams.d;
    *d_beams = (const BeamRec *)d;
    if (d_waves) *d_waves = (const BeamWave *)(d + nb);
    if (np) {  // a launch through several plasmas: their records and the beams' indices behind the two,
        // all four tables packed and sent as one copy
        std::vector<char> h(nb + nw + np + ni);
        if (nb) memcpy(h.data(), beams.data(), nb);
        if (nw) memcpy(h.data() + nb, waves.data(), nw);
        memcpy(h.data() + nb + nw, plasmas.data(), np);
        if (ni) memcpy(h.data() + nb + nw + np, beam_pl.data(), ni);
        HIPCK(hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, s));
        *d_plasmas = (const PlasmaRec *)(d + nb + nw);
        *d_beam_pl = (const int *)(d + nb + nw + np);
        return 0;
    }
    HIPCK(hipMemcpyAsync(d, beams.data(), nb, hipMemcpyHostToDevice, s));
    if (nw) HIPCK(hipMemcpyAsync(d + nb, waves.data(), nw, hipMemcpyHostToDevice, s));
    return 0;
}

// ---- the plasmas of a launch through several (torj_trace_beams_plasmas_device): the
// caller's two host tables; a null PlasmaSel is the launching handle's own plasma ----
struct PlasmaSel {
    int n;
    const torj_plasma_t *list;
    const int *beam_plasma;
};
static const PlasmaView kHandleView = {
    [](const void *h) { return ((const torj_plasma_s *)h)->device; },
    [](const void *h) {
        const torj_plasma_s *q = (const torj_plasma_s *)h;
        return PlasmaRec{q->d_coef, q->d_cellp, q->g, q->psi_prof_max};
    }};

// beams_plan, or beams_plasmas_plan when plasmas are given: argument errors, no HIP call
static int beams_any_plan(BeamsPlasmasPlan &pp, const torj_plasma_s *p, const PlasmaSel *ps, const torj_trace_cfg &cfg,
                          const BeamTables &bt, int n_psi, const LaunchPtrs &has) {
    if (!ps) return beams_plan(pp.bp, cfg, bt.n_beams, bt.beam_off, bt.omega, bt.mode, n_psi, has, launch_knobs(p));
    return beams_plasmas_plan(pp, cfg, ps->n, (const void *const *)ps->list, ps->beam_plasma, p->device, kHandleView,
                              bt.n_beams, bt.beam_off, bt.omega, bt.mode, n_psi, has, launch_knobs(p));
}

// the device state of every listed handle, then the launching one's (created on a
// handle's first GPU use: d_coef is null before).  All are on p's device (checked).
static int ensure_devices(torj_plasma_s *p, const PlasmaSel *ps) {
    if (ps)
        for (int j = 0; j < ps->n; j++)
            if (ensure_device(ps->list[j])) return -1;
    return ensure_device(p);
}

// k_trace_beams' instance: k_trace's set (launch_lanes).  BA: BeamsArgs, or BeamsPlArgs through several plasmas
template <class BA>
static void launch_beams(const BA &ba, const BeamsPlan &bp, hipStream_t s) {
    const dim3 grd((unsigned)bp.waves.size()), blk(64);
    if (bp.lpr == 16)
        with_depo_traj(bp.DM, bp.tr, [&](auto D, auto T) {
            if constexpr (D() != kDepoBinned)
                hipLaunchKernelGGL((k_trace_beams<1, D(), T(), 16, BA>), grd, blk, 0, s, ba);
        });
    else
        with_abs_depo_traj(ba.a.abs_model == 1 ? 1 : 0, bp.DM, bp.tr, [&](auto A, auto D, auto T) {
            if constexpr (A() <= 1) hipLaunchKernelGGL((k_trace_beams<A(), D(), T(), 1, BA>), grd, blk, 0, s, ba);
        });
}

// launch_post with the beams' kernels; the walk takes psi at the launch point from the
// handle's plasma (k_fit_depo itself) or from the ray's beam's
static void launch_fit_depo(const BeamsArgs &, const FitArgs &fa, dim3 grd, hipStream_t s) {
    hipLaunchKernelGGL(k_fit_depo, grd, dim3(64), fit_grid_lds(fa.n_psi), s, fa);
}
static void launch_fit_depo(const BeamsPlArgs &pa, const FitArgs &fa, dim3 grd, hipStream_t s) {
    hipLaunchKernelGGL(k_fit_depo_pl, grd, dim3(64), fit_grid_lds(fa.n_psi), s, fa, pa.beams, pa.n_beams, pa.plasmas,
                       pa.beam_pl);
}
template <class BA>
static int launch_post_beams(const BA &ba, const FitArgs &fa, hipStream_t s) {
    const dim3 grd(nblocks(ba.a.n, 64)), blk(64);
    with_abs(ba.a.abs_model, [&](auto A) {
        if constexpr (A() <= 1) hipLaunchKernelGGL((k_final_alpha_beams<A(), BA>), grd, blk, 0, s, ba);
    });
    launch_fit_depo(ba, fa, grd, s);
    hipLaunchKernelGGL(k_shell_sum_beams, dim3(fa.n_psi, ba.n_beams), dim3(256), 0, s, fa, ba.beams);
    HIPCK(hipGetLastError());
    return 0;
}

// one multi-beam launch on the caller's stream (the body of torj_trace_beams_device and, with `ps`, of
// torj_trace_beams_plasmas_device); the host tables are consumed before it returns
static int beams_trace_device(torj_plasma_t p, const PlasmaSel *ps, const torj_trace_cfg *cfg, const BeamTables &bt,
                              const RayIO &caller, int n_psi, void *stream) {
    if (!p || !cfg) return fail("bad plasma handle or cfg");
    const LaunchPtrs has = launch_ptrs(caller);
    BeamsPlasmasPlan pp;
    const BeamsPlan &bp = pp.bp;
    const bool fresh = !p->d_flags;  // n_cu is the device's only once ensure_device has run
    // argument errors need no device: before the NULL stream's fork touches one
    if (beams_any_plan(pp, p, ps, *cfg, bt, n_psi, has)) return -1;
    return on_caller_stream(p, stream, [&](hipStream_t s) -> int {
        if (p->timing) p->timing_calls++;
        if (ensure_devices(p, ps)) return -1;
        // (again with plasmas: their records hold device pointers, which exist only now)
        if ((fresh || ps) && beams_any_plan(pp, p, ps, *cfg, bt, n_psi, has)) return -1;
        RayIO io = caller;
        const int n = io.n = bp.n;  // the plan's: beam_off[n_beams]
        if (n == 0) return 0;
        if (cfg->absorption == 1 && ensure_gl_on_device(p->device)) return -1;
        if (bp.fit) {
            const size_t budget = ws_budget(p);
            if (bp.lay.bytes() > budget)
                return fail("multi-beam launch: the reference deposition's workspace for %d rays (%zu bytes) exceeds "
                            "the budget of %zu bytes (TORJ_WS_GB); trace the beams in separate calls",
                            n, bp.lay.bytes(), budget);
        }
        BeamsPlArgs pa{};
        BeamsArgs &ba = pa;
        torj_trace_cfg c1 = *cfg;  // (omega and mode are the beams'; any valid pair here)
        c1.omega = bt.omega[0], c1.mode = bt.mode[0];
        // (with plasmas a.coef, a.cellp and a.g are p's and unused: the beam's plasma record gives them)
        TraceArgs &a = ba.a = trace_args(p, c1, io);
        ba.n_beams = bt.n_beams;
        if (beams_upload(p, bp.beams, bp.waves, pp.plasmas, pp.beam_pl, s, &ba.beams, &ba.waves, &pa.plasmas,
                         &pa.beam_pl))
            return -1;
        FitArgs fa{};
        hipEvent_t ev[3];
        if (trace_prologue(p, bp, *cfg, io, n_psi, true, true, a, fa, ev, s)) return -1;
        auto run = [&](const auto &args) -> int {  // the trace and the phase after it, on either argument struct
            launch_beams(args, bp, s);
            HIPCK(hipGetLastError());
            if (ev[1]) HIPCK(hipEventRecord(ev[1], s));
            if (bp.fit && launch_post_beams(args, fa, s)) return -1;
            if (ev[2]) HIPCK(hipEventRecord(ev[2], s));
            return 0;
        };
        return ps ? run(pa) : run(ba);
    });
}

// ---- ray profiles (torj_ray_profile[_device]; torj_k_beams.hpp k_profile_beams, k_profile_pts) ----
// the call's own refusals and then the multi-beam plan's, on a cfg whose deposition is not
// read: no HIP call.  io: x0, N0, s0 and whichever of state, status, steps the caller gives.
static int profile_plan(BeamsPlasmasPlan &pp, const torj_plasma_s *p, const PlasmaSel *ps, const torj_trace_cfg *cfg,
                        const BeamTables &bt, const RayIO &io, int n_rows, const double *prof) {
    if (!p) return fail("torj_ray_profile: p is NULL");
    if (!cfg) return fail("torj_ray_profile: cfg is NULL");
    if (!prof) return fail("torj_ray_profile: prof is NULL");
    if (cfg->traj_stride < 1) return fail("torj_ray_profile: traj_stride = %d < 1", cfg->traj_stride);
    if (cfg->n_steps < 1) return fail("torj_ray_profile: n_steps = %d < 1", cfg->n_steps);
    if (n_rows != cfg->n_steps / cfg->traj_stride + 1)
        return fail("torj_ray_profile: n_rows = %d, but n_steps / traj_stride + 1 = %d", n_rows,
                    cfg->n_steps / cfg->traj_stride + 1);
    torj_trace_cfg c = *cfg;
    c.deposition = 0;
    const LaunchPtrs has = {io.x0 && io.N0, false, false, false, io.s0 != nullptr, false};
    return beams_any_plan(pp, p, ps, c, bt, 0, has);
}

template <class BA>
static int launch_profile(const BA &ba, const BeamsPlan &bp, double *prof, int n_rows, hipEvent_t ev[3],
                          hipStream_t s) {
    const dim3 grd((unsigned)bp.waves.size()), blk(64);
    if (bp.lpr == 16)
        hipLaunchKernelGGL((k_profile_beams<1, 16, BA>), grd, blk, 0, s, ba, prof);
    else if (ba.a.abs_model == 1)
        hipLaunchKernelGGL((k_profile_beams<1, 1, BA>), grd, blk, 0, s, ba, prof);
    else
        hipLaunchKernelGGL((k_profile_beams<0, 1, BA>), grd, blk, 0, s, ba, prof);
    HIPCK(hipGetLastError());
    if (ev[1]) HIPCK(hipEventRecord(ev[1], s));
    const dim3 grdB((unsigned)nblocks(ba.a.n, 64), (unsigned)std::min(n_rows, 65535));
    if (ba.a.abs_model == 1)
        hipLaunchKernelGGL((k_profile_pts<1, BA>), grdB, blk, 0, s, ba, prof, n_rows);
    else
        hipLaunchKernelGGL((k_profile_pts<0, BA>), grdB, blk, 0, s, ba, prof, n_rows);
    HIPCK(hipGetLastError());
    if (ev[2]) HIPCK(hipEventRecord(ev[2], s));
    return 0;
}

// one profile launch on the caller's stream (the body of torj_ray_profile_device): the table's
// NaN fill, the trace that stores (x, N, tau, s) per saved point, then the point kernel that
// fills the rest of every stored row.  The host tables are consumed before it returns.  No
// kernel of the launch sets a sticky flag (no psi grid, no work queue): torj_trace_check
// after it waits for the stream and reports what earlier launches left.  torj_timing: the
// trace is the trace phase, the point kernel the phase after it.
static int profile_device(torj_plasma_t p, const PlasmaSel *ps, const torj_trace_cfg *cfg, const BeamTables &bt,
                          const RayIO &caller, int n_rows, double *prof, void *stream) {
    BeamsPlasmasPlan pp;
    const BeamsPlan &bp = pp.bp;
    const bool fresh = !p || !p->d_flags;
    if (profile_plan(pp, p, ps, cfg, bt, caller, n_rows, prof)) return -1;
    return on_caller_stream(p, stream, [&](hipStream_t s) -> int {
        if (p->timing) p->timing_calls++;
        if (ensure_devices(p, ps)) return -1;
        if ((fresh || ps) && profile_plan(pp, p, ps, cfg, bt, caller, n_rows, prof)) return -1;
        RayIO io = caller;
        const int n = io.n = bp.n;
        if (n == 0) return 0;
        if (cfg->absorption == 1 && ensure_gl_on_device(p->device)) return -1;
        // the final state, status and steps the caller does not ask for: the handle's per-ray workspace
        if (!io.state || !io.status || !io.steps) {
            if (ensure_buf(p, p->ws, (size_t)n * (7 * sizeof(double) + 2 * sizeof(int)))) return -1;
            double *w = (double *)p->ws.d;
            if (!io.state) io.state = w;
            if (!io.status) io.status = (int *)(w + 7 * (size_t)n);
            if (!io.steps) io.steps = (int *)(w + 7 * (size_t)n) + n;
        }
        BeamsPlArgs pa{};
        BeamsArgs &ba = pa;
        torj_trace_cfg c1 = *cfg;  // (omega and mode are the beams'; any valid pair here)
        c1.omega = bt.omega[0], c1.mode = bt.mode[0];
        TraceArgs &a = ba.a = trace_args(p, c1, io);
        a.traj_stride = cfg->traj_stride;  // the rows' stride; a.traj stays null
        ba.n_beams = bt.n_beams;
        if (beams_upload(p, bp.beams, bp.waves, pp.plasmas, pp.beam_pl, s, &ba.beams, &ba.waves, &pa.plasmas,
                         &pa.beam_pl))
            return -1;
        // NaN, the bytes of the trace's own fill of traj
        HIPCK(hipMemsetAsync(prof, 0xFF, (size_t)n_rows * kProfCols * (size_t)n * sizeof(double), s));
        hipEvent_t ev[3];
        if (timing_begin(p, ev, s)) return -1;
        return ps ? launch_profile(pa, bp, prof, n_rows, ev, s) : launch_profile(ba, bp, prof, n_rows, ev, s);
    });
}

// ---- ray batches (trace_device): the beam in contiguous batches of nb
// rays, each its own trace_device_one; the batch's inputs gathered into and its
// outputs scattered from compact staging ----
static int trace_batched(torj_plasma_t p, const torj_trace_cfg *cfg, const RayIO &io, int nb, int n_psi,
                         hipStream_t s) {
    const int n = io.n, n_save = cfg->traj_stride > 0 && io.traj ? cfg->n_steps / cfg->traj_stride : 0;
    const size_t D = sizeof(double), B = (size_t)nb;
    // the staging's double arrays and their rows per ray, in the buffer's order;
    // status and steps (int) follow them
    enum { kX0, kN0, kXl, kW, kS0, kP, kSt, kTr, kNb };
    const int rows[kNb] = {3, 3, 3, 1, 1, 1, 7, 5 * n_save};
    size_t off[kNb + 1] = {0};  // in rows of B doubles
    for (int k = 0; k < kNb; k++) off[k + 1] = off[k] + (size_t)rows[k];
    if (ensure_buf(p, p->batch, off[kNb] * B * D + 2 * B * sizeof(int))) return -1;
    auto b = [&](int k) { return (double *)p->batch.d + off[k] * B; };
    RayIO bio = io;  // a batch's: staging rows; psi_grid, dP_shell and counters the caller's, shared by all
    bio.x0 = b(kX0), bio.N0 = b(kN0), bio.state = b(kSt), bio.P_dep = b(kP);
    bio.status = (int *)b(kNb), bio.steps = bio.status + B;
    bio.weights = io.weights ? b(kW) : nullptr, bio.x_launch = io.x_launch ? b(kXl) : nullptr;
    bio.s0 = io.s0 ? b(kS0) : nullptr, bio.traj = n_save ? b(kTr) : nullptr;
    for (int lo = 0; lo < n; lo += nb) {
        const int c = bio.n = std::min(nb, n - lo);
        // array k's rows of c rays from / to the caller's array h (rows of n rays, from ray lo)
        auto gather = [&](int k, const double *h) -> int {
            if (!h) return 0;
            HIPCK(hipMemcpy2DAsync(b(k), c * D, h + lo, (size_t)n * D, c * D, rows[k], hipMemcpyDeviceToDevice, s));
            return 0;
        };
        auto scatter = [&](double *h, int k) -> int {
            if (!h) return 0;
            HIPCK(hipMemcpy2DAsync(h + lo, (size_t)n * D, b(k), c * D, c * D, rows[k], hipMemcpyDeviceToDevice, s));
            return 0;
        };
        if (gather(kX0, io.x0) || gather(kN0, io.N0) || gather(kXl, io.x_launch) || gather(kW, io.weights) ||
            gather(kS0, io.s0))
            return -1;
        if (trace_device_one(p, cfg, bio, n_psi, s)) return -1;
        if (scatter(io.state, kSt) || scatter(io.P_dep, kP) || scatter(n_save ? io.traj : nullptr, kTr)) return -1;
        HIPCK(hipMemcpyAsync(io.status + lo, bio.status, c * sizeof(int), hipMemcpyDeviceToDevice, s));
        HIPCK(hipMemcpyAsync(io.steps + lo, bio.steps, c * sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// a trace on the caller's stream, whole or in ray batches (torj_trace_device_ex and every layer above it)
static int trace_device(torj_plasma_t p, const torj_trace_cfg *cfg, const RayIO &io, int n_psi, void *stream) {
    if (!p || !cfg) return fail("bad plasma handle or cfg");
    if (io.n <= 0) return 0;
    return on_caller_stream(p, stream, [&](hipStream_t s) {
        if (p->timing) p->timing_calls++;
        const bool fit = n_psi >= 2 && io.psi_grid && io.dP_shell && cfg->deposition == 1;
        // TORJ_SPLIT_BATCH=R (read per call; fixed-step absorbing beams): trace in
        // contiguous batches of R rays (a multiple of 64), each its own pipeline
        const long sb_rays =
            (cfg->integrator == 0 && cfg->absorption >= 1) ? env_long("TORJ_SPLIT_BATCH", 0) / 64 * 64 : 0;
        if ((fit || sb_rays > 0) && cfg->n_steps > 0 && launch_ptrs(io).rays) {
            const size_t per_ray =
                fit ? fit_bytes_per_ray((size_t)cfg->n_steps + 2, (size_t)n_psi, cfg->integrator == 1) : 0;
            if (ensure_device(p)) return -1;
            const size_t nb = batch_rays((size_t)io.n, per_ray, ws_budget(p), sb_rays);
            if (nb < (size_t)io.n) return trace_batched(p, cfg, io, (int)nb, n_psi, s);
        }
        return trace_device_one(p, cfg, io, n_psi, s);
    });
}
#endif  // TORJ_LAUNCH_PLAN_ONLY
