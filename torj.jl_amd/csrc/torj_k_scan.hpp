// torj_k_scan.hpp -- the split pipeline's optical-depth scan and its end:
// cold_replay (the NaN-alpha replay in the trajectory kernel's arithmetic),
// tau_scan_body, k_tau_scan[_counted] and k_split_final.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include "torj_args.hpp"
#include "torj_k_fused.hpp"  // deposit, wave_sum
#include "torj_k_traj.hpp"   // cold_step, kTraj*

// RK4 ray_segment from x, N over `k` steps (the NaN-alpha replay) in the
// arithmetic of the trajectory kernel that ran (sp.traj_mode): the same
// cold_step instance -- its stage-0 stencil with psi and its alpha-input
// stores, which change the compiler's fma contraction, here into row j = 0 of
// the ring slot sp.ain (no alpha kernel reads it any more: k_split_final runs
// after the last scan) -- read from the global table its tile falls back to
// (bit for bit the tile's values): the cell power form after k_traj_cell, the
// node tile's fallback after k_traj_tile, the node stencil otherwise (k_traj;
// k_traj_lds reads the same values from LDS, in a separately compiled kernel)
__device__ void cold_replay(const TraceArgs &a, const SplitArgs &sp, int i, double x[3], double N[3], int k) {
    const TileCell cg{a.cellp, nullptr, 0, 0, 0, 0};
    const TileCoef ng{a.coef, nullptr, 0, 0, 0, 0};
    ZBox zb;  // (unused: the replay stores no zero flags)
    TBox tb;
    for (int s = 0; s < k; s++) {
        double xn[3], Nn[3], psi;
        double *o_run = ain_row(a, sp, 0, i);  // every step into row 0
        if (sp.traj_mode == kTrajCell)
            cold_step<true, kTileNS, TileCell, true>(a, cg, sp, 0, i, x, N, xn, Nn, &psi, zb, false, tb, false, o_run);
        else if (sp.traj_mode == kTrajTile)
            cold_step<true, kTileNS, TileCoef, true>(a, ng, sp, 0, i, x, N, xn, Nn, &psi, zb, false, tb, false, o_run);
        else
            cold_step<true, kNF, const double *, true>(a, a.coef, sp, 0, i, x, N, xn, Nn, &psi, zb, false, tb, false, o_run);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            x[c] = xn[c];
            N[c] = Nn[c];
        }
    }
}

// COUNT: a counted launch (work words and counters); the uncounted scan
// carries neither the accumulators nor their loads (fewer registers beside the
// alpha waves it shares the SIMDs with)
template <int DEPO, bool TRAJ, bool COUNT>
__device__ __forceinline__ void tau_scan_body(const TraceArgs &a, const SplitArgs &sp) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    // counters [2..7] (include/torj_hip.h): Albajar or warm iwarm 1 meanings
    unsigned long long nsteps = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0;
    const int am = a.abs_model;
    // the group's flag word (SplitArgs::gflag; the workgroup is the group, so a
    // scalar load, safe as in k_alpha_pts): a flagged group's alpha waves stored
    // nothing -- its alphas are sp.zval and its work words 0, taken from here
    // (word 1: every ray flagged by the exact-zero proof, the alphas are sp.zval; word 2:
    // some by the tiny_alpha proof alone, sp.tval -- both 0 outside the test hooks)
    const unsigned gw = sp.gflag != nullptr ? group_word(sp.gflag, (int)blockIdx.x) : 0u;
    const bool gz = gw != 0u;
    const double gzv = gw == 1u ? sp.zval : sp.tval;
    if (i < a.n) {
        int steps = 0, st = ST_OK;
        double tau = 0.0, psi_a = 0.0, Pdep = 0.0;
        // the carry's loads issued together, the trajectory's stop word with them
        // (it used to wait behind sinfo's status): one memory latency, not two
        int sv = 0;
        const int tv = sp.tinfo[i];  // packed: steps and status written together
        if (sp.k0 > 0) {
            sv = sp.sinfo[i];
            tau = sp.stau[i];
            Pdep = sp.sPdep[i];
        }
        if constexpr (DEPO == kDepoBinned) psi_a = sp.spsi[i];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" ::"v"(tv), "v"(sv), "v"(tau), "v"(Pdep), "v"(psi_a));
#endif
        steps = info_steps(sv);
        st = info_status(sv);
        if (st == ST_OK) {
            const int tT = info_steps(tv), tS = info_status(tv);
            const double w = (DEPO == kDepoBinned && a.w) ? a.w[i] : 1.0;
            const double ds6 = a.ds / 6.0;
            double P = exp(-tau);  // bitwise the value the previous step computed
            DepoAcc dacc = {-1, 0.0};
            const int s_end = min(a.n_steps, sp.k0 + sp.kb);
            // the steps' alphas are loaded kScanBatch steps at a time (one memory
            // latency per batch instead of one per step: the scan is a serial
            // chain per lane); the loads stay inside the block's ring slot
            constexpr int kScanBatch = 4;
            bool done = false;
            for (int sb = steps; sb < s_end && !done; sb += kScanBatch) {
                double alb[kScanBatch][4];
#pragma unroll
                for (int v = 0; v < kScanBatch; v++) {
                    const size_t ov = (size_t)(min(sb + v, s_end - 1) - sp.k0) * 4 * a.n + i;
#pragma unroll
                    for (int q = 0; q < 4; q++) alb[v][q] = gz ? gzv : sp.alpha[ov + q * (size_t)a.n];
                }
#pragma unroll
                for (int v = 0; v < kScanBatch; v++) {
                    const int s = sb + v;
                    if (s >= s_end) break;
                    if (s >= tT) {  // the trajectory stopped before step s
                        if (tS == ST_NAN) st = ST_NAN;  // non-finite x / N at step s (ray_segment's `bad`)
                        done = true;
                        break;
                    }
                    const size_t o = (size_t)(s - sp.k0) * 4 * a.n + i;
                    const double al0 = (s == sp.nan_step && i % 3 == 0) ? (double)NAN : alb[v][0];
                    const double al1 = alb[v][1], al2 = alb[v][2], al3 = alb[v][3];
                    double acc_a = fma(1.0, al0, 0.0);
                    acc_a = fma(2.0, al1, acc_a);
                    acc_a = fma(2.0, al2, acc_a);
                    acc_a = fma(1.0, al3, acc_a);
                    const double taun = tau + ds6 * acc_a;
                    if (!isfinite(taun)) {  // alpha went non-finite: NAN at step s, state x_s
                        st = ST_NAN | 0x40;  // internal: the final state needs the replay
                        done = true;
                        break;
                    }
#pragma unroll
                    for (int q = 0; q < 4 && COUNT; q++) {
                        const unsigned wk = gz ? 0u : sp.awork[o + q * (size_t)a.n];
                        if (am == 1) {
                            c2 += wk & 1u;
                            c3 += (wk >> 1) & 3u;
                            c5 += (wk >> 3) & 3u;
                            c4 += (wk >> 5) & 2047u;
                            c6 += (wk >> 16) & 3u;
                            c7 += (wk >> 18) & 3u;
                        } else if (am == 2) {
                            const unsigned lrm = wk >> 21, passes = (wk >> 14) & 127u;
                            c2 += wk & 127u;
                            c3 += (wk >> 7) & 127u;
                            c4 += passes;
                            c5 += passes * lrm;
                            c6 += lrm;
                            c7 += lrm * lrm;
                        }
                    }
                    const double Pn = exp(-taun);
                    const double dP = P - Pn;
                    if constexpr (DEPO == kDepoSamples) {
                        if (s > 0) a.smp_dpds[smp_at(s, i, a.smp_rows)] = P * al0;
                    }
                    tau = taun;
                    P = Pn;
                    steps = s + 1;
                    nsteps++;
                    if constexpr (DEPO == kDepoBinned) {
                        const double psi_b = sp.psib[(size_t)(s - sp.k0) * a.n + i];
                        Pdep += deposit(a, dacc, psi_a, psi_b, dP, w);
                        psi_a = psi_b;
                    }
                    if constexpr (TRAJ) {
                        if (a.traj_stride > 0 && (steps % a.traj_stride) == 0)
                            a.traj[((size_t)(steps / a.traj_stride - 1) * 5 + 3) * a.n + i] = tau;
                    }
                    if (steps == tT && tS == ST_LEFT_PLASMA) {  // psi check first (src/solve.jl:174)
                        st = ST_LEFT_PLASMA;
                        done = true;
                        break;
                    }
                    if (a.chunk_steps > 0 && (steps % a.chunk_steps) == 0 && P < a.P_min) {  // :176
                        st = ST_ABSORBED;
                        done = true;
                        break;
                    }
                }
            }
            if constexpr (DEPO == kDepoBinned) depo_flush(a, dacc);
            sp.stau[i] = tau;
            sp.sPdep[i] = Pdep;
            if constexpr (DEPO == kDepoBinned) sp.spsi[i] = psi_a;
            sp.sinfo[i] = make_info(steps, st);
        }
    }
    if (COUNT) {
        const unsigned long long s0 = wave_sum(nsteps), s2 = wave_sum(c2), s3 = wave_sum(c3),
                                 s4 = wave_sum(c4), s5 = wave_sum(c5), s6 = wave_sum(c6),
                                 s7 = wave_sum(c7);
        if (threadIdx.x == 0) {
            atomicAdd(a.counters + 0, s0);
            atomicAdd(a.counters + 1, 4ull * s0);
            atomicAdd(a.counters + 2, s2);
            atomicAdd(a.counters + 3, s3);
            atomicAdd(a.counters + 4, s4);
            atomicAdd(a.counters + 5, s5);
            atomicAdd(a.counters + 6, s6);
            atomicAdd(a.counters + 7, s7);
        }
    }
}
template <int DEPO, bool TRAJ>
__global__ void __launch_bounds__(64) k_tau_scan(TraceArgs a, SplitArgs sp) {
    tau_scan_body<DEPO, TRAJ, false>(a, sp);
}
template <int DEPO, bool TRAJ>
__global__ void __launch_bounds__(64) k_tau_scan_counted(TraceArgs a, SplitArgs sp) {
    tau_scan_body<DEPO, TRAJ, true>(a, sp);
}

// final state, status and steps; trajectory samples past an earlier scan stop
template <int DEPO, bool TRAJ>
__global__ void __launch_bounds__(64) k_split_final(TraceArgs a, SplitArgs sp) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int sv = sp.sinfo[i], tv = sp.tinfo[i];
    const int steps = info_steps(sv), tT = info_steps(tv);
    int st = info_status(sv);
    double x[3], N[3];
    if (steps == tT && !(st & 0x40)) {  // the scan ran to the trajectory's end: its carry
#pragma unroll
        for (int c = 0; c < 3; c++) {
            x[c] = sp.tx[c * (size_t)a.n + i];
            N[c] = sp.tx[(3 + c) * (size_t)a.n + i];
        }
    } else {  // stopped earlier: from the chunk-boundary state (+ replay to step `steps`)
        const int cs = a.chunk_steps > 0 ? a.chunk_steps : 1 << 30;
        const int c0 = a.chunk_steps > 0 ? steps / cs : 0;
        const double *cb = sp.cbx + (size_t)c0 * 6 * a.n + i;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            x[c] = cb[c * (size_t)a.n];
            N[c] = cb[(3 + c) * (size_t)a.n];
        }
        cold_replay(a, sp, i, x, N, steps - c0 * (a.chunk_steps > 0 ? cs : 0));
        if constexpr (TRAJ) {  // samples the trajectory wrote past the stop
            if (a.traj_stride > 0)
                for (int k = steps / a.traj_stride; k < min(tT, a.n_steps) / a.traj_stride; k++)
                    for (int r = 0; r < 5; r++) a.traj[((size_t)k * 5 + r) * a.n + i] = NAN;
        }
    }
    st &= 0x3f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        a.state[c * a.n + i] = x[c];
        a.state[(3 + c) * a.n + i] = N[c];
    }
    a.state[6 * a.n + i] = sp.stau[i];
    a.status[i] = st;
    a.steps[i] = steps;
    const double Pdep = sp.sPdep[i];
    if (a.Pdep) a.Pdep[i] = Pdep;
    if constexpr (DEPO == kDepoBinned) {
        const double w = a.w ? a.w[i] : 1.0;
        atomicAdd(a.dP + a.n_psi, w * Pdep);  // sum_rays w P_dep
    }
}

