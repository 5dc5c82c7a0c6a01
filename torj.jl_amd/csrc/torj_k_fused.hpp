// torj_k_fused.hpp -- the fused trace kernels: the Gauss-Legendre table c_gl,
// shell deposition, ray_segment and the one-shot k_trace, the Tsit5 tables and
// ray_chunk_tsit5, the work queue (SchedCtl, k_trace_sched, k_sched_fold).
// c_gl, c_ts_a and c_ts_bt are defined here and nowhere else: only torj_hip.hip
// includes this file, so exactly one translation unit holds (and uploads) them.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include "torj_args.hpp"
#include "torj_fitdepo.hpp"

// ===========================================================================
// Gauss-Legendre table in constant memory (abs_Al_init, src/absorption.jl:1-7)
// ===========================================================================
__constant__ GLTable c_gl;

// psi shell j with grid[j] <= v < grid[j+1], clamped to [0, n-2]; identical
// result to a binary search on the grid array.
__device__ __forceinline__ int shell_of(const TraceArgs &a, double v) {
    // first guess as if the grid were uniform; accept it only if it brackets v,
    // else binary search: the result equals a binary search for any monotone grid
    const int nm2 = a.n_psi - 2;
    const double g0 = a.grid[0];
    int j = (int)floor((v - g0) * ((double)(a.n_psi - 1) / (a.grid[a.n_psi - 1] - g0)));
    j = j < 0 ? 0 : (j > nm2 ? nm2 : j);
    if (a.grid[j] <= v && (v < a.grid[j + 1] || j == nm2)) return j;
    int lo = 0, hi = a.n_psi - 1;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.grid[mid] <= v)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

struct DepoAcc {
    int cur;
    double acc;
};

// a lane's finished run of deposits into one shell: the wave's LDS histogram
// (flushed to dP once per queue visit) or, without one, a global atomic
__device__ __forceinline__ void depo_flush(const TraceArgs &a, const DepoAcc &d) {
    if (d.cur < 0) return;
    if (a.n_hist > 0) {
        extern __shared__ double lds_dyn[];
        atomicAdd(lds_dyn + a.hist_off + d.cur, d.acc);
    } else {
        atomicAdd(a.dP + d.cur, d.acc);
    }
}

__device__ __forceinline__ void depo_add(const TraceArgs &a, DepoAcc &d, int j, double v) {
    if (j == d.cur) {
        d.acc += v;
    } else {
        depo_flush(a, d);
        d.cur = j;
        d.acc = v;
    }
}

// power dP deposited over a step whose psi runs linearly pa -> pb
__device__ __forceinline__ double deposit(const TraceArgs &a, DepoAcc &d, double pa, double pb,
                                          double dP, double w) {
    if (!(dP != 0.0)) return 0.0;
    const double lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
    const double g0 = a.grid[0], gl = a.grid[a.n_psi - 1];
    if (hi == lo) {
        if (lo < g0 || lo > gl) return 0.0;
        depo_add(a, d, shell_of(a, lo), w * dP);
        return dP;
    }
    if (hi <= g0 || lo >= gl) return 0.0;
    const double span = hi - lo;
    double inside = 0.0;
    for (int j = shell_of(a, lo < g0 ? g0 : lo); j < a.n_psi - 1 && a.grid[j] < hi; j++) {
        const double gj = a.grid[j], gj1 = a.grid[j + 1];
        const double x0 = lo > gj ? lo : gj, x1 = hi < gj1 ? hi : gj1;
        if (x1 <= x0) continue;
        const double part = dP * ((x1 - x0) / span);
        depo_add(a, d, j, w * part);
        inside += part;
    }
    return inside;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Per-lane ray state carried through a segment of steps.
struct RayState {
    double x[3], N[3], tau, Pdep;
    int status, steps;
};

// A ray profile's table (torj_ray_profile, torj_k_beams.hpp): row `row` of ray i is
// prof[(row * kProfCols + c) * n + i].  The trace stores columns 0-7 of a saved
// point: x, N, tau and the arc length in the form the trajectory samples have it.
constexpr int kProfCols = 25;
__device__ __forceinline__ void profile_store(double *prof, const TraceArgs &a, int i, int row, const double x[3],
                                              const double N[3], double tau, int steps) {
    double *T = prof + (size_t)row * kProfCols * (size_t)a.n + i;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        T[c * (size_t)a.n] = x[c];
        T[(3 + c) * (size_t)a.n] = N[c];
    }
    T[6 * (size_t)a.n] = tau;
    T[7 * (size_t)a.n] = (a.s0 ? a.s0[i] : 0.0) + steps * a.ds;
}

// Integrate one ray from its current step to `s_end` (the make_ray loop,
// src/solve.jl:154-177): classic RK4 of sys!, optical depth, chunk-boundary
// termination, shell deposition, trajectory samples.  Shared by the one-shot
// and the work-queue kernels.
// LPR > 1: the ray's LPR lanes integrate it together (identical state in every
// lane; the absorption's node pairs are split between them) and lane sub = 0
// does the ray's stores.
// PROF (k_profile_beams): the saved points' (x, N, tau, s) into the rows of `prof`
// (profile_store) where TRAJ stores a sample; off, the code is what it was.
template <int ABS, int DEPO, bool TRAJ, int LPR = 1, bool PROF = false>
__device__ __forceinline__ void ray_segment(const TraceArgs &a, int i, double w, RayState &r,
                                            int s_end, AlbajarWork &work, int sub = 0, double *prof = nullptr) {
    static_assert(LPR == 1 || (ABS == 1 && DEPO != kDepoBinned), "lanes per ray: Albajar, no binning");
    const bool wr = LPR == 1 || sub == 0;
    const GLTable &gl = c_gl;
    double *x = r.x, *N = r.N;
    double tau = r.tau;
    double P = exp(-tau);  // bitwise the value the previous step computed
    double psi_a = 0.0;
    DepoAcc dacc = {-1, 0.0};
    if constexpr (DEPO != kDepoNone) psi_a = eval_one(a.coef, a.g, sqrt(x[0] * x[0] + x[1] * x[1]), x[2], F_PSI);
    if constexpr (DEPO == kDepoSamples) {
        if (r.steps == 0 && wr) {  // entry point: make_ray's dP_ds starts with 0 (src/solve.jl:151)
            a.smp_psi[smp_at(0, i, a.smp_rows)] = psi_a;
            a.smp_dpds[smp_at(0, i, a.smp_rows)] = 0.0;  // arc lengths are implicit: s_k = s0 + k ds (FitArgs::S)
        }
    }
    const double ds = a.ds, hds = 0.5 * a.ds, ds6 = a.ds / 6.0;
    for (int s = r.steps; s < s_end; s++) {
        // classic RK4 with a single RHS call site (one copy of the spline +
        // Albajar code live -> lower VGPR pressure)
        double acc[6] = {0, 0, 0, 0, 0, 0}, acc_a = 0.0, xt[3], Nt[3], k[6], al, al0 = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            xt[c] = x[c];
            Nt[c] = N[c];
        }
#pragma unroll 1
        for (int st = 0; st < 4; st++) {
            ray_rhs_m<ABS, LPR>(a.coef, a.g, a.k, gl, a.omega, a.mode, a.abs_model, xt, Nt, k, al,
                                wr ? &work : nullptr, sub);
            const double wgt = (st == 0 || st == 3) ? 1.0 : 2.0;
            const double h = (st < 2) ? hds : ds;
#pragma unroll
            for (int c = 0; c < 6; c++) acc[c] = fma(wgt, k[c], acc[c]);
            acc_a = fma(wgt, al, acc_a);
            if constexpr (DEPO == kDepoSamples) al0 = (st == 0) ? al : al0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                xt[c] = fma(h, k[c], x[c]);
                Nt[c] = fma(h, k[3 + c], N[c]);
            }
        }
        double xn[3], Nn[3];
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            xn[c] = x[c] + ds6 * acc[c];
            Nn[c] = N[c] + ds6 * acc[3 + c];
            bad |= !isfinite(xn[c]) || !isfinite(Nn[c]);
        }
        const double taun = tau + ds6 * acc_a;
        bad |= !isfinite(taun);
        if (bad) {
            r.status = ST_NAN;
            break;
        }
        const double Pn = exp(-taun);
        const double dP = P - Pn;
        if constexpr (DEPO == kDepoSamples) {
            // dP/ds at the saved point x_s = P_s alpha_approx(x_s) (src/solve.jl:171):
            // the stage-0 RHS of this step evaluated exactly that alpha (al0)
            if (s > 0 && wr) a.smp_dpds[smp_at(s, i, a.smp_rows)] = P * al0;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            x[c] = xn[c];
            N[c] = Nn[c];
        }
        tau = taun;
        P = Pn;
        r.steps = s + 1;
        const bool check = a.chunk_steps > 0 && (r.steps % a.chunk_steps) == 0;
        double psi_b = 0.0;
        if (DEPO != kDepoNone || check)
            psi_b = eval_one(a.coef, a.g, sqrt(x[0] * x[0] + x[1] * x[1]), x[2], F_PSI);
        if constexpr (DEPO == kDepoSamples) {
            if (wr) a.smp_psi[smp_at(r.steps, i, a.smp_rows)] = psi_b;
        }
        if constexpr (DEPO == kDepoBinned) {
            r.Pdep += deposit(a, dacc, psi_a, psi_b, dP, w);
            psi_a = psi_b;
        }
        if constexpr (TRAJ) {
            if (wr && a.traj_stride > 0 && (r.steps % a.traj_stride) == 0) {
                const size_t si = (size_t)(r.steps / a.traj_stride - 1);
                double *T = a.traj + si * 5 * (size_t)a.n + i;
                T[0] = x[0];
                T[(size_t)a.n] = x[1];
                T[2 * (size_t)a.n] = x[2];
                T[3 * (size_t)a.n] = tau;
                T[4 * (size_t)a.n] = (a.s0 ? a.s0[i] : 0.0) + r.steps * a.ds;
            }
        }
        if constexpr (PROF) {
            if (wr && a.traj_stride > 0 && (r.steps % a.traj_stride) == 0)
                profile_store(prof, a, i, r.steps / a.traj_stride, x, N, tau, r.steps);
        }
        if (check) {
            if (psi_b > a.psi_exit) {  // src/solve.jl:174
                r.status = ST_LEFT_PLASMA;
                break;
            }
            if (P < a.P_min) {  // src/solve.jl:176
                r.status = ST_ABSORBED;
                break;
            }
        }
    }
    r.tau = tau;
    if constexpr (DEPO == kDepoBinned) {
        depo_flush(a, dacc);
    }
}

__device__ __forceinline__ void load_start(const TraceArgs &a, int i, RayState &r) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        r.x[c] = a.x0[c * a.n + i];
        r.N[c] = a.N0[c * a.n + i];
    }
    r.tau = 0.0;
    r.Pdep = 0.0;
    r.status = ST_OK;
    r.steps = 0;
}

__device__ __forceinline__ void store_state(const TraceArgs &a, int i, const RayState &r) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
        a.state[c * a.n + i] = r.x[c];
        a.state[(3 + c) * a.n + i] = r.N[c];
    }
    a.state[6 * a.n + i] = r.tau;
    a.status[i] = r.status;
    a.steps[i] = r.steps;
    if (a.Pdep) a.Pdep[i] = r.Pdep;
}

__device__ __forceinline__ void flush_counters(const TraceArgs &a, unsigned long long steps,
                                               unsigned long long rhs, const AlbajarWork &work) {
    if (!a.counters) return;
    const unsigned long long s0 = wave_sum(steps);
    const unsigned long long s1 = wave_sum(rhs);
    const unsigned long long s2 = wave_sum((unsigned long long)work.n_active);
    const unsigned long long s3 = wave_sum((unsigned long long)work.n_harm);
    const unsigned long long s4 = wave_sum((unsigned long long)work.n_terms);
    const unsigned long long s5 = wave_sum((unsigned long long)work.n_zero);
    // [6]: Albajar's negligible-harmonic skips, or the warm model's sum of lrm
    // (each model leaves the other's field 0)
    const unsigned long long s6 = wave_sum((unsigned long long)(work.n_l + work.n_negl));
    const unsigned long long s7 = wave_sum((unsigned long long)(work.n_l2 + work.n_early));
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(a.counters + 0, s0);
        atomicAdd(a.counters + 1, s1);
        atomicAdd(a.counters + 2, s2);
        atomicAdd(a.counters + 3, s3);
        atomicAdd(a.counters + 4, s4);
        atomicAdd(a.counters + 5, s5);
        atomicAdd(a.counters + 6, s6);
        atomicAdd(a.counters + 7, s7);
    }
}

// One-shot kernel: LPR lanes per ray (1, or 16 for small beams whose rays
// would leave most SIMDs idle: the node pairs of the absorption integral are
// split between the ray's lanes), all steps in one pass.
template <int ABS, int DEPO, bool TRAJ, int LPR = 1>
__global__ void __launch_bounds__(TORJ_BLOCK, TORJ_MIN_WAVES) k_trace(TraceArgs a) {
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = gt / LPR, sub = gt % LPR;
    AlbajarWork work = {};
    unsigned long long steps = 0;
    if (i < a.n) {
        RayState r;
        load_start(a, i, r);
        const double w = (DEPO == kDepoBinned && a.w) ? a.w[i] : 1.0;
        ray_segment<ABS, DEPO, TRAJ, LPR>(a, i, w, r, a.n_steps, work, sub);
        if (sub == 0) {
            store_state(a, i, r);
            if constexpr (DEPO == kDepoBinned) atomicAdd(a.dP + a.n_psi, w * r.Pdep);  // sum_rays w P_dep
            steps = r.steps;
        }
    }
    flush_counters(a, steps, 4ull * steps, work);
}


// ---------------------------------------------------------------------------
// The reference's adaptive integration (integrator 1): one tspan chunk of
// solve(ODEProblem(sys!, u0, tspan; dtmax, abstol, reltol)) per visit
// (src/solve.jl:154-177), DifferentialEquations' default non-stiff method
// Tsit5 with OrdinaryDiffEq's PI controller and initial-step heuristic, on
// u = (x, N, P) with dP/ds = -P alpha.  The oracle restates the same
// algorithm (oracle/torj_oracle.c ts_ray); parity with DiffEq is unpinned.
// The seven stage vectors live in LDS (7 x 7 x 64 lanes x 8 B = 25 KB/wave).
// ---------------------------------------------------------------------------
__constant__ double c_ts_a[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {0.161, 0, 0, 0, 0, 0},
    {-0.008480655492356989, 0.335480655492357, 0, 0, 0, 0},
    {2.897153057105493, -6.359448489975075, 4.3622954328695815, 0, 0, 0},
    {5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525, 0, 0},
    {5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401,
     -0.028269050394068383, 0},
    {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081,
     2.324710524099774}};
__constant__ double c_ts_bt[7] = {-0.00178001105222577714, -0.0008164344596567469,
                                  0.007880878010261995,    -0.1447110071732629,
                                  0.5823571654525552,      -0.45808210592918697,
                                  0.015151515151515152};

template <int ABS>
__device__ __forceinline__ void rhs7(const TraceArgs &a, const double u[7], double du[7],
                                     AlbajarWork &work, unsigned long long &nrhs) {
    double al;
    ray_rhs_m<ABS, 1, false>(a.coef, a.g, a.k, c_gl, a.omega, a.mode, a.abs_model, u, u + 3, du, al, &work);
    du[6] = -u[6] * al;  // sys!: du[7] = -P alpha (src/solve.jl:113)
    nrhs++;
}

__device__ __forceinline__ double rms7(const double v[7]) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 7; q++) s = fma(v[q], v[q], s);
    return sqrt(s * (1.0 / 7.0));
}

template <int ABS, int DEPO, bool TRAJ>
__device__ void ray_chunk_tsit5(const TraceArgs &a, int i, double w, RayState &r, int ch,
                                double *kl, AlbajarWork &work, unsigned long long &nrhs) {
    // kl: this wave's LDS stage store, [stage][component][lane].  One RHS call
    // site: the loop walks the phases fsalfirst (st = -2), the initial-step
    // probe (st = -1) and the Tsit5 stages 1..6; all lanes stay in lockstep.
    const int lane = threadIdx.x & 63;
    auto K = [&](int st, int q) -> double & { return kl[(st * 7 + q) * 64 + lane]; };
    const double s_start = a.s0 ? a.s0[i] : 0.0;
    double t = (double)(ch - 1) * a.s_step + s_start;  // Float64(i-1)*s_step + s0
    const double tf = (double)ch * a.s_step + s_start;
    double u[7] = {r.x[0], r.x[1], r.x[2], r.N[0], r.N[1], r.N[2], r.tau};  // tau slot holds P
    double ut[7], dt = 0.0, dt0 = 0.0, d1 = 0.0, qold = 1e-4, q11 = 0.0;
    double psi_a = 0.0;
    if constexpr (DEPO == kDepoBinned) psi_a = eval_one(a.coef, a.g, sqrt(u[0] * u[0] + u[1] * u[1]), u[2], F_PSI);
    DepoAcc dacc = {-1, 0.0};
    int st = -2;
#pragma unroll 1
    for (;;) {
        if (st == -2) {
#pragma unroll
            for (int q = 0; q < 7; q++) ut[q] = u[q];
        } else if (st == -1) {
#pragma unroll
            for (int q = 0; q < 7; q++) ut[q] = fma(dt0, K(0, q), u[q]);
        } else {
            if (st == 1 && r.steps >= a.n_steps) {  // no room for another accepted step
                r.status = ST_MAX_STEPS;
                break;
            }
#pragma unroll
            for (int q = 0; q < 7; q++) {
                double acc = 0.0;
#pragma unroll 1
                for (int j = 0; j < st; j++) acc = fma(c_ts_a[st][j], K(j, q), acc);
                ut[q] = fma(dt, acc, u[q]);
            }
        }
        double kq[7];
        rhs7<ABS>(a, ut, kq, work, nrhs);
        if (st == -2) {  // fsalfirst; ode_determine_initdt, first half
#pragma unroll
            for (int q = 0; q < 7; q++) K(0, q) = kq[q];
            double v0[7], v1[7];
#pragma unroll
            for (int q = 0; q < 7; q++) {
                const double sk = a.abstol + fabs(u[q]) * a.reltol;
                v0[q] = u[q] / sk;
                v1[q] = kq[q] / sk;
            }
            const double d0 = rms7(v0);
            d1 = rms7(v1);
            dt0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : (d0 / d1) / 100.0;
            dt0 = fmin(dt0, a.ds);
            st = -1;
            continue;
        }
        if (st == -1) {  // ode_determine_initdt, second half (order 5)
            bool same = true;
            double v[7];
#pragma unroll
            for (int q = 0; q < 7; q++) {
                same &= (K(0, q) == kq[q]);
                v[q] = (kq[q] - K(0, q)) / (a.abstol + fabs(u[q]) * a.reltol);
            }
            if (same) {
                dt = 100.0 * dt0;
            } else {
                const double d2 = rms7(v) / dt0, m = fmax(d1, d2);
                const double dt1 = (m <= 1e-15) ? fmax(1e-6, dt0 * 1e-3) : pow(10.0, -(2.0 + log10(m)) / 5.0);
                dt = fmin(fmin(100.0 * dt0, dt1), a.ds);
            }
            if (!(t < tf)) break;
            dt = fmin(fabs(dt), tf - t);  // modify_dt_for_tstops!
            st = 1;
            continue;
        }
#pragma unroll
        for (int q = 0; q < 7; q++) K(st, q) = kq[q];
        if (st < 6) {
            st++;
            continue;
        }
        // ut = u_{n+1}; stage 6 is f(u_{n+1}) (FSAL): error estimate and step control
        double e[7];
        bool bad = false;
#pragma unroll
        for (int q = 0; q < 7; q++) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < 7; j++) acc = fma(c_ts_bt[j], K(j, q), acc);
            e[q] = dt * acc / (a.abstol + fmax(fabs(u[q]), fabs(ut[q])) * a.reltol);
            bad |= !isfinite(ut[q]);
        }
        if (bad) {
            r.status = ST_NAN;
            break;
        }
        const double EEst = rms7(e);
        double qq;
        if (EEst == 0.0) {
            qq = 0.1;
        } else {
            q11 = pow(EEst, 0.14);
            qq = fmax(0.1, fmin(5.0, (q11 / pow(qold, 0.08)) / 0.9));
        }
        if (EEst <= 1.0) {  // accept (qsteady_min = qsteady_max = 1)
            qold = fmax(EEst, 1e-4);
            const double dtnew = dt / qq;
            double tn = t + dt;
            if (fabs(tn - tf) < 100.0 * 2.220446049250313e-16 * fmax(fabs(t), fabs(tf))) tn = tf;
            const double Pa = u[6];
#pragma unroll
            for (int q = 0; q < 7; q++) {
                u[q] = ut[q];
                K(0, q) = K(6, q);
            }
            // the reference's ContinuousCallback(u[7] < 0, affect!): P is
            // projected to 0 (src/solve.jl:78-83,159-160), applied at the end of
            // the accepted step that crossed (DiffEq would root-find the crossing
            // inside the step; that location is unpinned here), and the FSAL
            // derivative follows: dP/ds = -P alpha = -0
            if (u[6] < 0.0) {
                u[6] = 0.0;
                K(0, 6) = -0.0;
            }
            t = tn;
            r.steps++;
            if constexpr (DEPO != kDepoNone) {
                const double psi_b = eval_one(a.coef, a.g, sqrt(u[0] * u[0] + u[1] * u[1]), u[2], F_PSI);
                if constexpr (DEPO == kDepoSamples) {
                    const size_t o = smp_at(r.steps, i, a.smp_rows);
                    a.smp_psi[o] = psi_b;
                    a.smp_dpds[o] = -K(0, 6);  // P alpha at the saved point (FSAL)
                    a.smp_s[o] = t;
                }
                if constexpr (DEPO == kDepoBinned) {
                    r.Pdep += deposit(a, dacc, psi_a, psi_b, Pa - u[6], w);
                    psi_a = psi_b;
                }
            }
            if constexpr (TRAJ) {
                if (a.traj_stride > 0 && (r.steps % a.traj_stride) == 0 &&
                    r.steps / a.traj_stride <= a.n_save) {
                    double *T = a.traj + (size_t)(r.steps / a.traj_stride - 1) * 5 * a.n + i;
                    T[0] = u[0];
                    T[(size_t)a.n] = u[1];
                    T[2 * (size_t)a.n] = u[2];
                    T[3 * (size_t)a.n] = -log(u[6]);
                    T[4 * (size_t)a.n] = t;
                }
            }
            dt = fmin(a.ds, dtnew);  // calc_dt_propose! (dtmax)
            if (!(t < tf)) break;
        } else {  // reject: step_reject_controller!(PIController)
            dt /= fmin(5.0, q11 / 0.9);
        }
        dt = fmin(fabs(dt), tf - t);  // modify_dt_for_tstops!
        st = 1;
    }
    if constexpr (DEPO == kDepoBinned) {
        depo_flush(a, dacc);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        r.x[c] = u[c];
        r.N[c] = u[3 + c];
    }
    r.tau = u[6];
    if (r.status == ST_OK) {  // chunk-end checks (src/solve.jl:174, :176)
        if (eval_one(a.coef, a.g, sqrt(u[0] * u[0] + u[1] * u[1]), u[2], F_PSI) > a.psi_exit)
            r.status = ST_LEFT_PLASMA;
        else if (u[6] < a.P_min)
            r.status = ST_ABSORBED;
    }
}

// Work-queue kernel (ready-queue of ray groups).
// The beam is cut into G groups of 64 rays (one wave each); a group's
// integration is done in visits of `cs` steps (the reference's termination
// chunk).  Waves pop a ready group, integrate one chunk, store its state and
// push it back (or retire it when all its rays are done).  Groups therefore
// migrate between SIMDs: SIMDs holding one wave (which runs a wave ~1.7x
// faster than a SIMD holding two) absorb more visits, evening out the 1.53
// waves/SIMD of a 1e5-ray beam.
//
// Queue: pops take head tickets h; h < G are the initial visits of group h;
// h >= G consume push position p = h - G, published as one 8-byte granule
// {tag = p + 1, group} (agent-scope release fence after the state stores, then
// a relaxed agent store).  Pop: relaxed agent poll of the granule, then an
// agent acquire fence before the state loads (MI355X_MICROARCH.md visibility
// rules).  Every spin is bounded (err flag after 120 s without a push or a
// retirement anywhere) and every wave exits once all G groups have retired,
// so the grid always drains.
struct SchedCtl {
    unsigned head, tail, finished, err;
};

constexpr unsigned kGroupExit = 0xffffffffu;
constexpr unsigned long long kStallTicks = 120ull * 100000000ull;  // 120 s at 100 MHz

// returns the group index; bit 31 set = first visit (state from x0/N0)
__device__ __forceinline__ unsigned sched_pop(SchedCtl *ctl, unsigned long long *slots, unsigned S,
                                              unsigned G) {
    unsigned g = kGroupExit;
    if (threadIdx.x == 0) {
        const unsigned h = __hip_atomic_fetch_add(&ctl->head, 1u, __ATOMIC_RELAXED,
                                                  __HIP_MEMORY_SCOPE_AGENT);
        if (h < G) {
            g = h | 0x80000000u;
        } else {
            const unsigned long long pos = h - G;
            unsigned long long *slot = slots + (pos % S);
            // stall watchdog: no push and no retirement anywhere in the grid for
            // kStallTicks of the 100 MHz realtime clock (a long chunk of heavy
            // physics is progress elsewhere, not a stall)
            unsigned long long t_prog = __builtin_amdgcn_s_memrealtime();
            unsigned prog = 0xffffffffu;
            for (unsigned spins = 0;; spins++) {
                unsigned long long v = __hip_atomic_load(slot, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT);
                if ((v >> 32) == pos + 1) {
                    g = (unsigned)v;
                    break;
                }
                if (__hip_atomic_load(&ctl->finished, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= G) {
                    v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    g = ((v >> 32) == pos + 1) ? (unsigned)v : kGroupExit;
                    break;
                }
                if ((spins & 255u) == 0) {
                    const unsigned pr =
                        __hip_atomic_load(&ctl->tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) +
                        __hip_atomic_load(&ctl->finished, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                    if (pr != prog) {
                        prog = pr;
                        t_prog = now;
                    } else if (now - t_prog > kStallTicks) {  // never hang the device
                        __hip_atomic_store(&ctl->err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                }
                __builtin_amdgcn_s_sleep(4);
            }
        }
    }
    g = __shfl(g, 0, 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return g;
}

__device__ __forceinline__ void sched_publish_begin() {
    // every lane's state stores are issued by this one wave: drain them, then
    // write back the XCD L2 (agent release) before the granule / counter
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int ABS, int DEPO, bool TRAJ, int INTEG>
__global__ void __launch_bounds__(64, ABS >= 2 ? TORJ_WARM_MIN_WAVES : TORJ_MIN_WAVES) k_trace_sched(TraceArgs a, SchedCtl *ctl,
                                                                     unsigned long long *slots,
                                                                     unsigned S, int G, int cs) {
    extern __shared__ double lds_k[];  // integrator 1: Tsit5 stage vectors of this wave
    AlbajarWork work = {};
    unsigned long long steps = 0, nrhs = 0;
    double *hist = lds_k + a.hist_off;  // binned deposition: this wave's shell histogram
    if constexpr (DEPO == kDepoBinned) {
        for (int k = threadIdx.x; k < a.n_hist; k += 64) hist[k] = 0.0;
    }
    for (;;) {
        const unsigned t = sched_pop(ctl, slots, S, (unsigned)G);
        if (t == kGroupExit) break;
        const unsigned g = t & 0x7fffffffu;
        const int i = (int)g * TORJ_GROUP + threadIdx.x;
        bool alive = false;
        if (threadIdx.x < TORJ_GROUP && i < a.n) {
            RayState r;
            int ch = 0;
            if (t & 0x80000000u) {
                load_start(a, i, r);
                if constexpr (INTEG == 1) r.tau = 1.0;  // the tau slot carries P
            } else {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    r.x[c] = a.state[c * a.n + i];
                    r.N[c] = a.state[(3 + c) * a.n + i];
                }
                r.tau = a.state[6 * a.n + i];
                r.status = a.status[i];
                r.steps = a.steps[i];
                r.Pdep = a.Pdep ? a.Pdep[i] : 0.0;
                if constexpr (INTEG == 1) ch = a.chunk[i];
            }
            const double w = (DEPO == kDepoBinned && a.w) ? a.w[i] : 1.0;
            if constexpr (INTEG == 0) {
                if (r.status == ST_OK && r.steps < a.n_steps) {
                    const int s0 = r.steps;
                    const int s_end = min(a.n_steps, (s0 / cs + 1) * cs);
                    ray_segment<ABS, DEPO, TRAJ>(a, i, w, r, s_end, work);
                    steps += (unsigned long long)(r.steps - s0);
                    nrhs += 4ull * (unsigned long long)(r.steps - s0);
                    alive = r.status == ST_OK && r.steps < a.n_steps;
                    if constexpr (DEPO == kDepoBinned) {
                        if (!alive) atomicAdd(a.dP + a.n_psi, w * r.Pdep);  // sum_rays w P_dep
                    }
                }
                store_state(a, i, r);
            } else {
                const bool ran = r.status == ST_OK && ch < a.n_chunks;
                if (ran) {
                    const int s0 = r.steps;
                    if constexpr (DEPO == kDepoSamples) {
                        if (ch == 0) {  // entry point (src/solve.jl:151)
                            const size_t o = smp_at(0, i, a.smp_rows);
                            a.smp_psi[o] = eval_one(a.coef, a.g, sqrt(r.x[0] * r.x[0] + r.x[1] * r.x[1]), r.x[2], F_PSI);
                            a.smp_dpds[o] = 0.0;
                            a.smp_s[o] = a.s0 ? a.s0[i] : 0.0;
                        }
                    }
                    ch++;
                    ray_chunk_tsit5<ABS, DEPO, TRAJ>(a, i, w, r, ch, lds_k, work, nrhs);
                    steps += (unsigned long long)(r.steps - s0);
                    alive = r.status == ST_OK && ch < a.n_chunks;
                    if constexpr (DEPO == kDepoBinned) {
                        if (!alive) atomicAdd(a.dP + a.n_psi, w * r.Pdep);
                    }
                }
                a.chunk[i] = ch;
                // the tau slot carries P while the ray runs and tau = -ln P once it
                // has finished -- converted on the visit that finished it only (a
                // finished ray of a live group is reloaded and stored again)
                if (ran && !alive) r.tau = -log(r.tau);  // final state carries tau = -ln P
                store_state(a, i, r);
            }
        }
        const bool any_alive = __any(alive);
        if constexpr (DEPO == kDepoBinned) {  // the visit's shell sums: LDS -> dP
            if (a.n_hist > 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int k = threadIdx.x; k < a.n_hist; k += 64) {
                    const double v = hist[k];
                    if (v != 0.0) {
                        atomicAdd(a.dP + k, v);
                        hist[k] = 0.0;
                    }
                }
            }
        }
        sched_publish_begin();
        if (threadIdx.x == 0) {
            if (any_alive) {
                const unsigned long long pos = __hip_atomic_fetch_add(&ctl->tail, 1u, __ATOMIC_RELAXED,
                                                                      __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(slots + (pos % S), ((pos + 1) << 32) | (unsigned long long)g,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                __hip_atomic_fetch_add(&ctl->finished, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    flush_counters(a, steps, nrhs, work);
}

// a work-queue launch's outcome into the handle's sticky flags (bit 1 stall
// watchdog, bit 2 not every group retired); read by torj_trace_check
__global__ void k_sched_fold(const SchedCtl *ctl, unsigned G, int *flags) {
    int f = 0;
    if (ctl->err) f |= 2;
    if (ctl->finished != G) f |= 4;
    if (f) atomicOr(flags, f);
}
