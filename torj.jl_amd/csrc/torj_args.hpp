// torj_args.hpp -- what the trace kernels and their launches agree on: the
// argument blocks TraceArgs and SplitArgs, the deposition modes, the packed
// steps | status word, and the compile-time launch-shape defaults (each with
// the measurement that chose it).
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include "torj_math.hpp"

struct TraceArgs {
    const double *coef;
    const double *cellp;  // the coefficients' per-cell power form (torj_math.hpp cell_power_table)
    Grid g;
    Consts k;
    double omega;
    int mode;
    double ds;
    int n_steps;
    int chunk_steps;
    double psi_exit;
    double P_min;
    int n;
    const double *x0;  // 3 x n
    const double *N0;  // 3 x n
    const double *w;   // n or null
    double *state;     // 7 x n
    int *status;
    int *steps;
    int n_psi;
    const double *grid;
    double *dP;  // n_psi + 1
    double *Pdep;
    int traj_stride;
    int n_save;
    double *traj;  // n_save x 4 x n
    unsigned long long *counters;
    double *smp_psi;   // DEPO == 2: psi(x_k), torj::smp_at layout
    double *smp_dpds;  // DEPO == 2: P_k alpha(x_k), torj::smp_at layout
    double *smp_s;     // DEPO == 2: arc length s_k, torj::smp_at layout
    size_t smp_rows;   // rows per ray of the smp_at layout (n_steps + 2)
    int abs_model;     // 1 Albajar, 2 warm weakly relativistic, 3 warm fully relativistic
    const double *s0;  // n: arc length at the entry point (null: 0)
    // integrator 1 (the reference's adaptive solve)
    double abstol, reltol, s_step;
    int n_chunks;
    int *chunk;  // n: chunks done (work-queue visits carry it)
    // binned deposition in the work-queue kernel: per-wave LDS histogram of
    // n_hist shells at dynamic-LDS offset hist_off (doubles); 0 = global atomics
    int n_hist, hist_off;
};

// the adaptive queue kernel's Tsit5 stage vectors in dynamic LDS (k_trace_sched)
constexpr int kTsLds = 7 * 7 * 64;  // doubles per wave

// DEPO modes of the trace kernels
constexpr int kDepoNone = 0, kDepoBinned = 1, kDepoSamples = 2;

// the fused kernels' launch shape: lanes per workgroup of k_trace, and the
// waves per SIMD its and k_trace_sched's register budget allows
#ifndef TORJ_BLOCK
#define TORJ_BLOCK 256
#endif
#ifndef TORJ_MIN_WAVES
#define TORJ_MIN_WAVES 2
#endif
// rays per work-queue group (one wave's lanes; fewer leaves the upper lanes idle)
#ifndef TORJ_GROUP
#define TORJ_GROUP 64
#endif
// warm kernels: one wave per SIMD -- the 512-VGPR budget holds the warm
// tensor without spills (C5: 458 vs 505 ms at two waves per SIMD)
#ifndef TORJ_WARM_MIN_WAVES
#define TORJ_WARM_MIN_WAVES 1
#endif

// alpha-input buffers in flight in the split pipeline (the ring: torj_split.hpp)
constexpr int kSplitRing = 4;

constexpr int kAinF = 5;  // X, Y, |N|^2, N_par, ln Te (warm: X, Y, |N|, N_par, Te, 1 / |dD/dN|: kAinFW)
constexpr int kAinFW = 6;

struct SplitArgs {
    double *ain;          // [j][stage][f][n]: this block's alpha inputs, nf fields
    double *alpha;        // [j][stage][n]
    unsigned *awork;      // [j][stage][n] (null unless counted): alpha work counts; Albajar: bit 0 active,
                          // bits 1-2 harmonics, 3-4 exact-zero harmonics, 5-15 Bessel terms,
                          // 16-17 negligible harmonics;
                          // warm: bits 0-6 larmornumber tests, 7-13 Faddeeva evaluations,
                          // 14-20 warmdisp passes, 21-23 Larmor order
    double *psib;         // binned deposition: psi at the end of step k0 + j, [j][n]
    double *cbx;          // [c][6][n]: x, N at chunk boundary c (steps = c * chunk_steps)
    double *tx;           // [6][n]: the trajectory kernel's carry
    int *tinfo;           // steps | status << 24: the trajectory kernel's stop (one store)
    double *stau, *spsi, *sPdep;  // the scan's carry
    int *sinfo;           // steps | status << 24: the scan's stop
    unsigned char *zflag;  // per ray, this block (ring slot): 1 = Albajar alpha provably +-0 at every
                           // stage point the trajectory kernel stored (zero_box_flag), 2 = the same by
                           // tiny_box_flag alone (tiny_alpha below), 0 = neither; null: off
    double zval;           // what a fully flagged alpha wave writes: 0, or NaN under the test hook
                           // TORJ_TEST_ZFLAG_NAN=1 (the flagged waves then stop their rays NAN)
    unsigned *gflag;       // per 64-ray group, this block (ring slot): 1 = every ray of the group carries
                           // zflag 1, 2 = every ray carries 1 or 2, 0 = some ray carries 0.  Written once per wave by the trajectory kernel; the group's alpha
                           // waves end on it and the scan takes zval for the group's alphas (nothing is
                           // stored for them).  Null: off (TORJ_ALPHA_GFLAG=0, or zflag null)
    int k0, kb;           // block: steps [k0, k0 + kb)
    int nf;               // alpha input fields per point: kAinF (Albajar) or kAinFW (warm)
    int tile_cap;         // k_traj_tile: most nodes a wave stages (<= kTileNodes)
    double tile_margin;   // k_traj_tile: the box's margin in units of the block's path, (kb + 1) ds
    int traj_mode;        // the trajectory kernel (kTrajL2 .. kTrajCell): the NaN-alpha replay uses its arithmetic
    int nan_step;         // test hook (TORJ_TEST_NAN_ALPHA_STEP, default -1): the scan reads alpha as NaN
                          // at this step for every third ray, to exercise the NaN-alpha replay
    unsigned long long *defer;  // warm: the block's points with lrm > 3, (js << 32) | i, for k_alpha_warm_big
    unsigned *defer_cnt;        // warm: their count (this block's slot, zeroed per launch)
    int defer_lrm;              // warm: points with lrm above this are deferred (3; TORJ_WARM_DEFER_LRM
                                // lowers it: a test sends every point through the deferred path)
    int zlatch;                 // the trajectory kernel's dead-box latch (traj_run; TORJ_ZBOX_LATCH=0 in the
                                // environment turns it off).  In the struct's tail padding: the kernels'
                                // arguments after a SplitArgs keep their offsets
    double tiny_alpha;          // > 0: the trajectory kernel also flags a ray whose alpha is a zero over the
                                // block by the tiny_alpha bound (tiny_box_flag; the Gauss-Legendre table's
                                // tiny_alpha, m^-1); 0: zero_box_flag alone (split_tiny_alpha says when).
                                // Such a ray's zflag byte is 2, and the word of a group that is wholly
                                // flagged but not wholly by zero_box_flag is 2: every reader tests != 0
    double tval;                // zval's twin for a byte / word 2: 0, or NaN under the test hook
                                // TORJ_TEST_TFLAG_NAN (TORJ_TEST_ZFLAG_NAN keeps to the exact-zero proof)
};

// Word g of SplitArgs::gflag for the wave's own group (g wave-uniform), read
// through the constant address space so that it is a scalar load, issued without
// a vector-memory round trip.  Only for a word that an earlier kernel wrote and
// no kernel running now writes (the scalar cache is not coherent with vector
// stores): the readers say why that holds.
__device__ __forceinline__ unsigned group_word(const unsigned *gflag, int g) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) unsigned *const_ptr;
    return ((const_ptr)(unsigned long long)gflag)[g];
#else
    return gflag[g];
#endif
}

// steps | status << 24: split launches need n_steps < kSplitMaxSteps (the
// fused kernels have no such limit and take longer traces)
constexpr int kSplitMaxSteps = 1 << 24;
__device__ __forceinline__ int info_steps(int v) { return v & 0xffffff; }
__device__ __forceinline__ int info_status(int v) { return (unsigned)v >> 24; }
__device__ __forceinline__ int make_info(int steps, int st) { return steps | (st << 24); }

// the split pipeline's kernels (torj_k_traj.hpp, torj_k_alpha.hpp)
#ifndef TORJ_AIN_TRAJ_MATH  // 1: the trajectory kernel stores |N| and Te for k_alpha_pts (not |N|^2, ln Te)
#define TORJ_AIN_TRAJ_MATH 0
#endif
#ifndef TORJ_TRAJ_WAVES
#define TORJ_TRAJ_WAVES TORJ_MIN_WAVES
#endif
#ifndef TORJ_ALPHA_WAVES  // k_alpha_pts' waves per SIMD bound (6: <= 80 VGPRs; round 5 with the tiny-alpha
// skip, alternating: 40.01 / 40.01 ms against 40.23 / 40.12 at 4, 96 VGPRs; 8 spills: 48.6 ms)
#define TORJ_ALPHA_WAVES 6
#endif
#ifndef TORJ_ALPHA_UNROLL  // node pairs per iteration of the alpha kernel's node loop (ILP)
#define TORJ_ALPHA_UNROLL 1
#endif
#ifndef TORJ_TILE_NODES
#define TORJ_TILE_NODES 256  // 12 KB of LDS per wave
#endif
constexpr int kTileNodes = TORJ_TILE_NODES;
#ifndef TORJ_TILE_CELLS
#define TORJ_TILE_CELLS 20  // 15 KB of LDS per wave
#endif
constexpr int kTileCells = TORJ_TILE_CELLS;

// where the trajectory kernel reads the field coefficients (torj_k_traj.hpp), and
// the doubles per node of k_traj_lds' whole-grid table
enum { kTrajL2 = 0, kTrajLds = 1, kTrajTile = 2, kTrajCell = 3 };
constexpr int kTrajLdsNS = 6;

#ifndef TORJ_TRAJ_LDS_WAVES
#define TORJ_TRAJ_LDS_WAVES 1
#endif
#ifndef TORJ_TRAJ_TILE_WAVES
#define TORJ_TRAJ_TILE_WAVES 2
#endif

// ---- a multi-beam launch (torj_k_beams.hpp; planned by torj_launch.hpp beams_plan) ----
// beam b: rays lo .. hi - 1 of the concatenated arrays, its own frequency and mode
struct BeamRec {
    double omega;
    Consts k;
    int mode;
    int lo, hi;
};
// wave w of the launch: its beam and the first ray it carries (a wave never mixes beams)
struct BeamWave {
    int beam, first;
};
// the trace's arguments (omega, k, mode unused: the wave's beam gives them; dP: row 0
// of n_beams rows of n_psi + 1) and the two tables, device-resident
struct BeamsArgs {
    TraceArgs a;
    const BeamRec *beams;
    const BeamWave *waves;
    int n_beams;
};

// ---- a multi-beam launch through several plasmas (torj_k_beams.hpp; planned by
// torj_launch.hpp beams_plasmas_plan) ----
// one listed plasma: what TraceArgs (coef, cellp, g) and the ray entry (psi_max) take from a handle
struct PlasmaRec {
    const double *coef;
    const double *cellp;
    Grid g;
    double psi_max;
};
// BeamsArgs (a.coef, a.cellp, a.g unused: the beam's plasma gives them) and two more
// device-resident tables: the listed plasmas' records, and beam b's index into them
struct BeamsPlArgs : BeamsArgs {
    const PlasmaRec *plasmas;
    const int *beam_pl;  // n_beams
};
