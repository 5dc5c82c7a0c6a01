// torj_k_traj.hpp -- the split pipeline's trajectory kernels: the zero box,
// cold_step, traj_run / traj_body and k_traj, k_traj_lds, k_traj_tile,
// k_traj_cell.  Needs torj_args.hpp and the math headers only -- never
// torj_k_fused.hpp: torj_traj.hip compiles this file without the fused kernels
// and their __constant__ tables.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include "torj_args.hpp"
#include "torj_fitdepo.hpp"

// ---------------------------------------------------------------------------
// Split RK4 path: trajectory and optical depth as separate, overlapped kernels
// (fixed-step RK4, Albajar).
//
// In sys! (src/solve.jl:112-114) dx/ds and dN/ds are gradΛ!(x, N) alone: the
// absorption only drives u[7].  So the trajectory of every ray is fixed before
// any alpha is known, and the 4 x n_steps alpha evaluations of a ray are
// independent of each other -- the step's chain is the cheap cold RHS, the
// expensive part is embarrassingly parallel.  Per block of B steps:
//   k_traj      one lane per ray: the cold RK4 steps (the same arithmetic as
//               ray_segment), writing each stage's alpha inputs (X, Y, |N|,
//               N_par, Te), psi per step, chunk-boundary states, trajectory
//               samples; stops LEFT_PLASMA / NAN exactly as ray_segment;
//   k_alpha_pts one lane per (ray, step, stage): abs_albajar_fast at the
//               stored inputs -- a fully occupied grid, no step chain;
//   k_tau_scan  one lane per ray, in step order: tau += ds/6 (a0 + 2a1 + 2a2 +
//               a3) with ray_segment's fma order, P = exp(-tau), the ABSORBED
//               check at chunk boundaries (after T's psi check, as the
//               reference), make_ray's dP/ds samples, binned deposition, tau in
//               the trajectory samples;
// then k_split_final assembles the final state (a ray the scan stops earlier
// than the trajectory takes its chunk-boundary state, or replays the last
// steps when alpha itself went non-finite).  k_traj of block b+1 runs on the
// caller's stream while k_alpha_pts / k_tau_scan of block b run on a second
// stream: the trajectory waves (~1.5 per SIMD on a 1e5-ray beam) and the alpha
// waves share the SIMDs.  A wave of k_alpha_pts holds the 64 rays of a 64-ray
// group at one (step, stage): the same lanes as the fused kernel's wave there,
// so the per-wave Bessel-level ballot and every alpha are the same bits.
// ---------------------------------------------------------------------------
// The alpha-input box of one ray over a block (round 6): the range of ln Te,
// Y, N_par^2 and N_perp^2 over every stage point the trajectory kernel stored.
// zero_box_flag proves from it that abs_albajar_fast_body returns +-0 at every
// one of them -- all Te < 20 eV, or each harmonic m = 2, 3 absent (m Y <
// sqrt(1 - N_par^2)) or an exact zero (every node's exp(mu (1 - gamma))
// underflows: gamma_min > 1 + 760 / mu, the natural-exponent form of harm_geom's
// ymax < kZeroYmax = -1096 in base 2 (torj_math.hpp; 760 log2(e) = 1096.4), with
// gamma_min >= m Y / (1 + |N_par|)
// on the resonance gamma - N_par u_par = m Y, |u_par| <= gamma) -- the early
// settle of abs_albajar_fast_body (and its exact-zero test), which returns +0
// there, decided for a whole block with relative margins of 1e-9 against
// their roundings, and only inside the ranges in which the body itself stays
// finite: 1e-100 < Y < 1e100 (r = m Y / sqrt(1 - N_par^2) is squared), ln Te <
// 300 (albajar_finish squares 1 / mu), N_perp^2 > 1e-9 |N|^2 and N_par^2 < 1 -
// 1e-9 (1 - 1e-6 with TORJ_NODE_GAMMA_LIN 0, whose gamma_min^2 cancels r^2 /
// (1 - N_par^2)); any NaN or infinite input refuses.  k_alpha_pts then writes 0 for a wave whose 64 rays all
// carry the flag instead of evaluating it (42 % of its waves settle early on the
// headline beam).
// (ZBox, zero_box_add and zero_box_flag live in torj_math.hpp after
// abs_albajar_fast_body, whose early settle they restate: host and device, so
// that tests/test_skip_proofs_host.py can sweep them against it on CPU)

#ifndef TORJ_TRAJ_AIN_STEP
#define TORJ_TRAJ_AIN_STEP 1
#endif
// row `row` of the block's alpha inputs (a row: one stage of one step, nf fields of n rays) at ray i
__device__ __forceinline__ double *ain_row(const TraceArgs &a, const SplitArgs &sp, int row, int i) {
    return sp.ain + ((size_t)row * sp.nf) * a.n + i;
}
// One cold RK4 step of ray_segment's arithmetic (plasma_point with ln Te, as
// the absorbing kernels evaluate it); STORE: this step's alpha inputs -> ain.
// PSI: stage 0's stencil also sums psi at x (the step's start), returned in
// *psi_x -- the psi the previous step's end needs (traj_run), bit for bit the
// eval_one at that point.
template <bool STORE, int NS = kNF, class CS = const double *, bool PSI = false>
__device__ __forceinline__ bool cold_step(const TraceArgs &a, CS coef,
                                          const SplitArgs &sp, int j, int i, const double x[3],
                                          const double N[3], double xn[3], double Nn[3],
                                          double *psi_x, ZBox &zb, bool zon, TBox &tb, bool ton,
                                          double *&o_run) {
    const double hds = 0.5 * a.ds, ds6 = a.ds / 6.0;
    double acc[6] = {0, 0, 0, 0, 0, 0}, xt[3], Nt[3], k[6];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        xt[c] = x[c];
        Nt[c] = N[c];
    }
    // the cell-tiled kernel's trims (round 11): stage st's alpha inputs go to ain
    // + ((j * 4 + st) * nf) * n + i -- per stage a 64-bit product of a lane's j
    // (two v_mul_lo_u32 and a v_mad_u64_u32, quarter rate) -- which is one row
    // of nf * n further at every stage, step after step: the caller's pointer
    // o_run, at row j * 4 on entry, moves on by a row per stage (ain_row;
    // TORJ_TRAJ_AIN_STEP) and replaces j; and the dispersion's unused reciprocal
    // sits behind a wave-uniform branch
    constexpr bool kCellTrim = IsTileCell<CS>::value;
#pragma unroll 1
    for (int st = 0; st < 4; st++) {
        PlasmaPoint p;
        if constexpr (PSI) {
            // stage 0 with the sixth field (a branch around whole evaluations: a
            // per-field gate inside the stencil split its blocks and spilled)
            if (st == 0) {
                plasma_point<true, NS, CS, true>(coef, a.g, a.k, xt, p);
                *psi_x = p.psi;
            } else {
                plasma_point<true, NS>(coef, a.g, a.k, xt, p);
            }
        } else {
            plasma_point<true, NS>(coef, a.g, a.k, xt, p);
        }
        double Npar, inv;
        dispersion_grad<kCellTrim>(p, Nt, a.mode, k, &Npar, &inv);
        if constexpr (STORE) {
            double *o;
            if constexpr (kCellTrim && TORJ_TRAJ_AIN_STEP) {
                o = o_run;
                o_run += (size_t)sp.nf * a.n;
            } else {
                o = sp.ain + ((size_t)(j * 4 + st) * sp.nf) * a.n + i;
            }
            const double N2 = Nt[0] * Nt[0] + Nt[1] * Nt[1] + Nt[2] * Nt[2];
            if (zon) {
                zero_box_add(zb, p.lnTe, p.Y, Npar, N2);
                if (ton) {  // (ton implies zon; wave-uniform as well)
                    // X = n_e Cx over again (the same bits as p.X) from an opaque copy of
                    // n_e: a use of p.X's own product here, a block ahead of the dispersion's
                    // arithmetic, kept the compiler from contracting 1 - X and X - 1 into
                    // fmas there as it always had, and k_traj_cell's trajectories moved by
                    // an ulp against every earlier build
                    double ne = p.ne;
#if defined(__HIP_DEVICE_COMPILE__)
                    asm("" : "+v"(ne));
#endif
                    tiny_box_add(zb, tb, ne * a.k.Cx, N2);
                }
            }
            o[0] = p.X;
            o[(size_t)a.n] = p.Y;
            o[3 * (size_t)a.n] = Npar;
            if (sp.nf > kAinF) {  // the warm inputs as ray_rhs_m<2 / 3> forms them
                o[2 * (size_t)a.n] = sqrt(N2);
                o[4 * (size_t)a.n] = exp(p.lnTe);
                o[kAinF * (size_t)a.n] = inv;
            } else if constexpr (TORJ_AIN_TRAJ_MATH) {
                // |N| and Te by the functions k_alpha_pts would apply (the same
                // bits), on the trajectory chain, which has slack once the alpha
                // chain is the pipeline's critical one
                o[2 * (size_t)a.n] = sqrt_pos(N2);
                o[4 * (size_t)a.n] = exp_fast<true>(p.lnTe);
            } else {
                // |N|^2 and ln Te: k_alpha_pts takes the square root and the
                // exponential (the same functions ray_rhs applies), off the
                // latency-bound trajectory chain and onto the parallel alpha lanes
                o[2 * (size_t)a.n] = N2;
                o[4 * (size_t)a.n] = p.lnTe;
            }
        }
        const double wgt = (st == 0 || st == 3) ? 1.0 : 2.0;
        const double h = (st < 2) ? hds : a.ds;
#pragma unroll
        for (int c = 0; c < 6; c++) acc[c] = fma(wgt, k[c], acc[c]);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            xt[c] = fma(h, k[c], x[c]);
            Nt[c] = fma(h, k[3 + c], N[c]);
        }
    }
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        xn[c] = x[c] + ds6 * acc[c];
        Nn[c] = N[c] + ds6 * acc[3 + c];
        bad |= !isfinite(xn[c]) || !isfinite(Nn[c]);
    }
    return bad;
}

// Where the trajectory kernel reads the field coefficients:
//   kTrajL2    the global array through L1 / L2 (any grid);
//   kTrajLds   the whole grid staged in LDS (6 fp64 per node, 161 KB for a 56 x 56
//              grid: one workgroup of up to 8 waves per CU);
//   kTrajTile  per wave and block, only the tile of nodes its rays can reach in
//              the block's kb steps (|dx/ds| = 1, so within (kb + 1) ds of where
//              they start), a few KB: the kernel is no longer capped at one
//              workgroup per CU, and its waves share every SIMD with the alpha
//              waves.  A stencil outside the tile reads the global array (the
//              same values: results bit-identical in every mode).
//   kTrajCell  per wave and block, the tile of CELLS its rays can reach, each
//              cell's bicubic in power form (torj_math.hpp cell_sums: 28 fma per
//              field with its gradient against the node stencil's 44, no basis
//              weights); the same fallback to the global cell table.
// (the enum and kTrajLdsNS: torj_args.hpp; the choice: torj_split.hpp split_traj_mode)
static_assert(kTrajLdsNS == kTileNS, "LDS layouts");

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// the cell index axis_setup gives a coordinate (monotone in x)
__device__ __forceinline__ int cell_index(double x, double x1, double xn, double invh, int n) {
    const int i = (int)floor((clampd(x, x1, xn) - x1) * invh);
    return i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
}

#ifndef TORJ_TRAJ_PREWAIT
#define TORJ_TRAJ_PREWAIT 1
#endif
// the dead-box latch of traj_run (0: never compiled in; 1: on unless
// TORJ_ZBOX_LATCH=0 in the environment, read per call: SplitArgs::zlatch), and
// the loop trips after which a wave looks at its boxes' flags
#ifndef TORJ_ZBOX_LATCH
#define TORJ_ZBOX_LATCH 1
#endif
#ifndef TORJ_ZLATCH_TRIP0
#define TORJ_ZLATCH_TRIP0 1
#endif
#ifndef TORJ_ZLATCH_TRIP1
#define TORJ_ZLATCH_TRIP1 16
#endif
constexpr int kZLatchTrip0 = TORJ_ZLATCH_TRIP0, kZLatchTrip1 = TORJ_ZLATCH_TRIP1;
// the trajectory steps of one ray over the block, from its carry (x, N, steps)
template <int DEPO, bool TRAJ, int NS, class CS>
__device__ __forceinline__ void traj_run(const TraceArgs &a, const SplitArgs &sp, CS coef, int i,
                                         double x[3], double N[3], int steps, int st) {
    if (sp.k0 == 0) {
        if constexpr (DEPO != kDepoNone) {
            const double psi0 = eval_one<NS>(coef, a.g, sqrt(x[0] * x[0] + x[1] * x[1]), x[2], F_PSI);
            sp.spsi[i] = psi0;  // the scan's psi_a at step 0
            if constexpr (DEPO == kDepoSamples) {
                a.smp_psi[smp_at(0, i, a.smp_rows)] = psi0;
                a.smp_dpds[smp_at(0, i, a.smp_rows)] = 0.0;
            }
        }
    }
    const int s_end = min(a.n_steps, sp.k0 + sp.kb);
    // psi at the end of step s - 1 is psi at x_s, which step s's stage 0 sums
    // from its own stencil (cold_step<PSI>): the end-of-step work that needs it
    // (make_ray's psi sample, the binned deposition's psi, the psi_exit check)
    // runs one iteration late, before step s's outcome is looked at, so the
    // order of stops is ray_segment's (psi check, then the next step's NaN);
    // the block's last step takes the one eval_one left.  A ray stopped by the
    // check has stored step s's alpha inputs too -- beyond its steps, so
    // k_alpha_pts and the scan never read them.
    auto step_end = [&](int k, double psi_b) -> bool {  // after step k (steps = k + 1)
        const int sk = k + 1;
        if constexpr (DEPO == kDepoSamples) a.smp_psi[smp_at(sk, i, a.smp_rows)] = psi_b;
        if constexpr (DEPO == kDepoBinned) sp.psib[(size_t)(k - sp.k0) * a.n + i] = psi_b;
        return a.chunk_steps > 0 && (sk % a.chunk_steps) == 0 && psi_b > a.psi_exit;  // src/solve.jl:174
    };
    const int s_first = steps;
    bool pending = false;  // step steps - 1 still needs its psi
    // (a value and a flag, not a pointer: a local behind a conditional pointer
    // lived in scratch, 56 B per lane, and slowed the kernel by ~14 %)
    ZBox zb;
    bool zon = sp.zflag != nullptr;  // wave-uniform: the stages' branch around zero_box_add
    const bool zlatch = TORJ_ZBOX_LATCH && zon && sp.zlatch != 0;
    // The block tiny box (torj_math.hpp TBox, tiny_box_flag): with SplitArgs::tiny_alpha
    // > 0 a ray's flag is "zero_box_flag or tiny_box_flag" -- alpha an exact zero, or a
    // zero because harmonic 3 is dismissed by the tiny_alpha bound, at every stage
    // point of the block.  k_alpha_pts and the scan read the same byte and word.
    TBox tb;
    const bool ton = zon && sp.tiny_alpha > 0.0;
    auto box_flag = [&]() -> bool {
        return zero_box_flag(zb) || (ton && tiny_box_flag(zb, tb, a.omega, a.mode, sp.tiny_alpha));
    };
    int trips = 0;  // of the wave's step loop (uniform, unlike s)
#if defined(__HIP_DEVICE_COMPILE__) && TORJ_TRAJ_PREWAIT
    // every load before the step loop complete here (s_waitcnt vmcnt(0)): the
    // compiler otherwise waits at the loop header for the carry's loads, every
    // step, and on gfx9 vmcnt counts stores too -- each step would then wait for
    // its own last stage's alpha-input stores to reach memory
    __builtin_amdgcn_s_waitcnt(0x0F70);
#endif
    double *o_run = ain_row(a, sp, (s_first - sp.k0) * 4, i);  // cold_step's store pointer (the cell kernel)
    for (int s = s_first; s < s_end; s++) {
        double xn[3], Nn[3], psi_x;
        const bool bad = cold_step<true, NS, CS, true>(a, coef, sp, s - sp.k0, i, x, N, xn, Nn, &psi_x, zb, zon, tb, ton, o_run);
        if (pending) {
            pending = false;
            if (step_end(s - 1, psi_x)) {
                st = ST_LEFT_PLASMA;
                break;
            }
        }
        if (bad) {
            st = ST_NAN;
            break;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            x[c] = xn[c];
            N[c] = Nn[c];
        }
        steps = s + 1;
        const bool check = a.chunk_steps > 0 && (steps % a.chunk_steps) == 0;
        pending = DEPO != kDepoNone || check;
        if constexpr (TRAJ) {
            if (a.traj_stride > 0 && (steps % a.traj_stride) == 0) {
                double *T = a.traj + (size_t)(steps / a.traj_stride - 1) * 5 * a.n + i;
                T[0] = x[0];
                T[(size_t)a.n] = x[1];
                T[2 * (size_t)a.n] = x[2];
                T[4 * (size_t)a.n] = (a.s0 ? a.s0[i] : 0.0) + steps * a.ds;
            }
        }
        if (check) {
            double *cb = sp.cbx + (size_t)(steps / a.chunk_steps) * 6 * a.n + i;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                cb[c * (size_t)a.n] = x[c];
                cb[(3 + c) * (size_t)a.n] = N[c];
            }
        }
        // The dead-box latch, over "zero_box_flag or tiny_box_flag" (box_flag; the
        // second is monotone for the same reason, tests/test_tiny_box_host.py).
        // zero_box_flag is monotone: a further point only
        // raises lte, yhi, np2 and chk's NaN and lowers ylo and perp, and each of
        // its conditions only gets harder that way, so a box whose flag is false
        // stays false to the end of the block (swept on the CPU by
        // tests/test_zbox_latch_host.py).  Once no lane still in the loop has a
        // true flag, the rest of the block's zero_box_add calls decide nothing:
        // they stop, and these lanes' boxes are poisoned through chk so that they
        // write flag 0.  A lane that left the loop earlier is not active here and
        // keeps its own box.  Even off the proof the latch could only turn a 1
        // into a 0, which k_alpha_pts answers by evaluating the zero.
        if (zlatch && zon) {
            trips++;
            if (trips == kZLatchTrip0 || trips == kZLatchTrip1) {
                if (!__any(box_flag())) {
                    zero_box_kill(zb);
                    zon = false;
                }
            }
        }
    }
    double invR;
    if (pending && step_end(steps - 1, eval_one<NS>(coef, a.g, cyl_radius(x, invR), x[2], F_PSI)))
        st = ST_LEFT_PLASMA;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        sp.tx[c * (size_t)a.n + i] = x[c];
        sp.tx[(3 + c) * (size_t)a.n + i] = N[c];
    }
    sp.tinfo[i] = make_info(steps, st);
    if (sp.zflag != nullptr) {
        // byte 1: the exact-zero proof; 2: the tiny_alpha proof alone (SplitArgs::tiny_alpha)
        const bool zf0 = zero_box_flag(zb);
        const bool zf = zf0 || box_flag();
        sp.zflag[i] = zf0 ? 1 : (zf ? 2 : 0);
        // the group's word (SplitArgs::gflag): the lanes here are the wave's rays
        // with steps in this block, reconverged behind the step loop; a lane that
        // left in traj_body carries flag 1 by definition, so the `all` over these
        // is the group's.  Every one of them stores the same word to the same
        // address: the wave's one store, whichever lanes are left
        // (word 1 only when every one of them has the exact-zero proof: a ray that
        // left earlier counts as such, as its byte says)
        if (sp.gflag != nullptr) sp.gflag[i >> 6] = __all(zf) ? (__all(zf0) ? 1u : 2u) : 0u;
    }
}


template <int DEPO, bool TRAJ, int MODE>
__device__ __forceinline__ void traj_body(const TraceArgs &a, const SplitArgs &sp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double x[3] = {0, 0, 0}, N[3] = {0, 0, 0};
    int steps = 0, st = ST_OK;
    bool live = i < a.n;
    if (live) {
        if (sp.k0 == 0) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                x[c] = a.x0[c * a.n + i];
                N[c] = a.N0[c * a.n + i];
                sp.cbx[c * (size_t)a.n + i] = x[c];
                sp.cbx[(3 + c) * (size_t)a.n + i] = N[c];
            }
        } else {
            const int v = sp.tinfo[i];
            steps = info_steps(v);
            st = info_status(v);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                x[c] = sp.tx[c * (size_t)a.n + i];
                N[c] = sp.tx[(3 + c) * (size_t)a.n + i];
            }
        }
        // a ray the scan has stopped (ABSORBED) needs no more trajectory.  sinfo is
        // written by k_tau_scan on another stream while this kernel may run, so the
        // read can be stale.  INVARIANT: this early-out only saves work, it never
        // decides an output -- a stale OK just traces steps nobody reads (the scan
        // stopped first; k_split_final rebuilds the state from the chunk-boundary
        // copy and the scan's carry).  Keep it that way: tests/test_gpu_split.py
        // test_split_serial_equals_overlapped holds both orders bit-identical.
        live = st == ST_OK && !(sp.k0 > 0 && info_status(sp.sinfo[i]) != ST_OK);
        // a ray without trajectory steps in this block needs no alpha in it
        if (!live && sp.zflag) sp.zflag[i] = 1;
    }
    // A wave without a live ray never reaches traj_run's store of the group's
    // word: it writes the 1 here, in every mode (the tile kernels return
    // wave-uniformly below, the others lane by lane).  The ring slot still holds
    // the word of kRing blocks ago, so a skipped write is a wrong flag, not a
    // missing one.  (i < n: a wave past the last group has no word)
    if (sp.gflag != nullptr && !__any(live) && i < a.n) sp.gflag[i >> 6] = 1u;
    if constexpr (MODE == kTrajTile) {
        // one wave per workgroup: the wave's live rays' (R, Z) box, widened by
        // the path the block can take, and its nodes staged in LDS
        __shared__ __attribute__((aligned(16))) double s_tile[kTileNodes * kTileNS];
        const double R = sqrt(x[0] * x[0] + x[1] * x[1]);
        const double inf = __builtin_inf();
        const double rmin = wave_min(live ? R : inf), rmax = wave_max(live ? R : -inf);
        const double zmin = wave_min(live ? x[2] : inf), zmax = wave_max(live ? x[2] : -inf);
        if (!(rmin <= rmax && zmin <= zmax)) return;  // no live ray in the wave (wave-uniform)
        const double m = (double)(sp.kb + 1) * a.ds * sp.tile_margin;
        const int iR0 = cell_index(rmin - m, a.g.R1, a.g.Rn, a.g.invhR, a.g.nR),
                  iR1 = cell_index(rmax + m, a.g.R1, a.g.Rn, a.g.invhR, a.g.nR),
                  iZ0 = cell_index(zmin - m, a.g.Z1, a.g.Zn, a.g.invhZ, a.g.nZ),
                  iZ1 = cell_index(zmax + m, a.g.Z1, a.g.Zn, a.g.invhZ, a.g.nZ);
        TileCoef tc{a.coef, s_tile, iR0, iZ0, iR1 - iR0 + 4, iZ1 - iZ0 + 4};
        if (tc.tw * tc.th > sp.tile_cap) {
            tc.tw = tc.th = 0;  // too wide for the tile: every stencil from global memory
        } else {
            const int mR = a.g.nR + 2, cnt = tc.tw * tc.th * kTileNS;
            for (int k = threadIdx.x; k < cnt; k += 64) {
                const int node = k / kTileNS, f = k - node * kTileNS;
                const int zr = node / tc.tw, rr = node - zr * tc.tw;
                s_tile[k] = a.coef[((size_t)(iZ0 + zr) * mR + iR0 + rr) * kNF + f];
            }
        }
        __syncthreads();
        if (!live) return;
        traj_run<DEPO, TRAJ, kTileNS>(a, sp, tc, i, x, N, steps, st);
    } else if constexpr (MODE == kTrajCell) {
        // the cells the wave's live rays can reach in the block (the node tile's
        // box, by cell), their power-form records staged in LDS
        __shared__ __attribute__((aligned(16))) double s_cell[kTileCells * kCellLds];
        const double R = sqrt(x[0] * x[0] + x[1] * x[1]);
        const double inf = __builtin_inf();
        const double rmin = wave_min(live ? R : inf), rmax = wave_max(live ? R : -inf);
        const double zmin = wave_min(live ? x[2] : inf), zmax = wave_max(live ? x[2] : -inf);
        if (!(rmin <= rmax && zmin <= zmax)) return;  // no live ray in the wave (wave-uniform)
        const double m = (double)(sp.kb + 1) * a.ds * sp.tile_margin;
        const int iR0 = cell_index(rmin - m, a.g.R1, a.g.Rn, a.g.invhR, a.g.nR),
                  iR1 = cell_index(rmax + m, a.g.R1, a.g.Rn, a.g.invhR, a.g.nR),
                  iZ0 = cell_index(zmin - m, a.g.Z1, a.g.Zn, a.g.invhZ, a.g.nZ),
                  iZ1 = cell_index(zmax + m, a.g.Z1, a.g.Zn, a.g.invhZ, a.g.nZ);
        // the box is wave-uniform: scalar registers for the copy's loop
        const int cR0 = __builtin_amdgcn_readfirstlane(iR0), cZ0 = __builtin_amdgcn_readfirstlane(iZ0);
        const int cw = __builtin_amdgcn_readfirstlane(iR1 - iR0 + 1), ch = __builtin_amdgcn_readfirstlane(iZ1 - iZ0 + 1);
        TileCell tc{a.cellp, s_cell, cR0, cZ0, cw, ch};
        if (cw * ch > sp.tile_cap) {
            tc.cw = tc.ch = 0;  // too wide for the tile: every cell from global memory
        } else {
            // one cell record (48 x 16 B) per pass, lanes 0..47 (measured: four
            // loads in flight per lane over the flattened tile is no faster)
            const int cR = a.g.nR - 1;
            const Dbl2 *src = reinterpret_cast<const Dbl2 *>(a.cellp);
            Dbl2 *dst = reinterpret_cast<Dbl2 *>(s_cell);
            for (int zr = 0; zr < ch; zr++)
                for (int rr = 0; rr < cw; rr++)
                    if (threadIdx.x < kCellRec / 2)
                        dst[(zr * cw + rr) * (kCellLds / 2) + threadIdx.x] =
                            src[((size_t)(cZ0 + zr) * cR + cR0 + rr) * (kCellRec / 2) + threadIdx.x];
        }
        __syncthreads();
        if (!live) return;
        traj_run<DEPO, TRAJ, kTileNS>(a, sp, tc, i, x, N, steps, st);
    } else if constexpr (MODE == kTrajLds) {
        extern __shared__ __attribute__((aligned(16))) double s_coef[];
        const int nodes = (a.g.nR + 2) * (a.g.nZ + 2);
        for (int k = threadIdx.x; k < nodes * kTrajLdsNS; k += blockDim.x)
            s_coef[k] = a.coef[(size_t)(k / kTrajLdsNS) * kNF + k % kTrajLdsNS];
        __syncthreads();
        if (!live) return;
        traj_run<DEPO, TRAJ, kTrajLdsNS>(a, sp, (const double *)s_coef, i, x, N, steps, st);
    } else {
        if (!live) return;
        traj_run<DEPO, TRAJ, kNF>(a, sp, (const double *)a.coef, i, x, N, steps, st);
    }
}

template <int DEPO, bool TRAJ>
__global__ void __launch_bounds__(64, TORJ_TRAJ_WAVES) k_traj(TraceArgs a, SplitArgs sp) {
    traj_body<DEPO, TRAJ, kTrajL2>(a, sp);
}
template <int DEPO, bool TRAJ>
__global__ void __launch_bounds__(512, TORJ_TRAJ_LDS_WAVES) k_traj_lds(TraceArgs a, SplitArgs sp) {
    traj_body<DEPO, TRAJ, kTrajLds>(a, sp);
}
template <int DEPO, bool TRAJ>
__global__ void __launch_bounds__(64, TORJ_TRAJ_TILE_WAVES) k_traj_tile(TraceArgs a, SplitArgs sp) {
    traj_body<DEPO, TRAJ, kTrajTile>(a, sp);
}
// k_traj_cell is compiled in a translation unit of its own (torj_traj.hip)
// without machine-level loop-invariant code motion: hoisted out of the step
// loop, the kernel arguments' loads and constants held 208 VGPRs and spilled 15
// SGPRs; left in place, 160 VGPRs and no spill, so two trajectory waves and two
// 80-VGPR alpha waves share a SIMD.  The alpha kernel
// keeps the hoisting (without it +3.4 % VALU and +49 % SALU).
// TORJ_TRAJ_OWN_TU=1 (the Makefile, for torj_hip.hip): k_traj_cell is only
// declared and comes from torj_traj.hip; 0 (torj_traj.hip itself, and a
// single-TU build of torj_hip.hip): defined here.  That unit includes this
// file without torj_k_fused.hpp, so the __constant__ tables c_gl, c_ts_a and
// c_ts_bt exist in torj_hip.hip's unit alone -- a kernel that reads one belongs
// in a header torj_traj.hip does not include.
#ifndef TORJ_TRAJ_OWN_TU
#define TORJ_TRAJ_OWN_TU 0
#endif
// measurement knob: a VGPR budget for the cell kernel between the 2- and 3-wave
// bounds (176: two trajectory waves and two 80-VGPR alpha waves share a SIMD)
#ifdef TORJ_TRAJ_CELL_VGPR
#define TORJ_TRAJ_CELL_ATTR __attribute__((amdgpu_num_vgpr(TORJ_TRAJ_CELL_VGPR)))
#else
#define TORJ_TRAJ_CELL_ATTR
#endif
#if !TORJ_TRAJ_OWN_TU
template <int DEPO, bool TRAJ>
__global__ void __launch_bounds__(64, TORJ_TRAJ_TILE_WAVES) TORJ_TRAJ_CELL_ATTR k_traj_cell(TraceArgs a, SplitArgs sp) {
    traj_body<DEPO, TRAJ, kTrajCell>(a, sp);
}
#else
// defined and instantiated in torj_traj.hip (its own compile flags, above)
template <int DEPO, bool TRAJ>
__global__ void __launch_bounds__(64, TORJ_TRAJ_TILE_WAVES) TORJ_TRAJ_CELL_ATTR k_traj_cell(TraceArgs a, SplitArgs sp);
#endif
