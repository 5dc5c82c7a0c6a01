// torj_k_beams.hpp -- the multi-beam forms of the one-shot trace and of the
// kernels around it: B beams' rays concatenated, each beam with its own
// frequency and mode and its own row of dP_shell (BeamsArgs, torj_args.hpp; the
// tables come from torj_launch.hpp beams_plan).  k_trace_beams runs one wave per
// workgroup, wave w the rays its table entry names: the lanes of a wave are
// k_trace's on that beam alone, and the beam's omega, Consts and mode are
// uniform over the wave (scalar loads by blockIdx, SGPRs as k_trace's kernel
// arguments are).  The device functions are k_trace's, unchanged.
// Beams that go through differing plasmas (BeamsPlArgs; torj_launch.hpp
// beams_plasmas_plan): beam b is traced through the listed plasma beam_pl[b], whose
// coefficients, cell table and grid replace the handle's in the trace's arguments.  A
// wave never mixes beams, so its plasma is wave-uniform like its omega: k_trace_beams
// loads the record by blockIdx (scalar loads, SGPRs).  The kernels after the trace run
// one lane per ray and look the ray's beam up, then that beam's plasma.
// Each kernel is written once for both: a template on the argument struct, BeamsArgs
// or BeamsPlArgs (beam_args is overloaded on the two), or, where the arguments are
// loose, on a trailing pack that is empty or the two plasma tables (beam_plasma
// likewise); k_fit_depo_pl is the plasma form of k_fit_depo itself.  The bodies repeat
// their single-beam kernels' (k_trace, k_final_alpha, k_ray_entry, k_fit_depo) and are
// not one function with them: a shared __forceinline__ body is optimised on its own
// before it is inlined and gave those kernels other registers and schedules
// (profiles/r14/kernels_asm.txt).  A fix to one of the four is made there and here.
// Ray profiles (torj_ray_profile[_device]): k_profile_beams, k_trace_beams' body storing
// (x, N, tau, s) per saved point, and k_profile_pts, the rest of each stored row.
// (a slice of torj_hip.hip: included after `using namespace torj`)
#pragma once
#include "torj_args.hpp"
#include "torj_entry.hpp"
#include "torj_k_depo.hpp"
#include "torj_k_fused.hpp"
#include "torj_k_points.hpp"

// the beam of ray i: the first whose hi exceeds i (empty beams own no ray);
// i < beams[n_beams - 1].hi
__device__ __forceinline__ int beam_of(const BeamRec *beams, int n_beams, int i) {
    int lo = 0, hi = n_beams - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (beams[mid].hi > i)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// the trace's arguments as beam b's single launch would have them, ray indices global
__device__ __forceinline__ TraceArgs beam_args(const BeamsArgs &ba, int b, const BeamRec &br) {
    TraceArgs a = ba.a;
    a.omega = br.omega, a.k = br.k, a.mode = br.mode;
    if (a.dP) a.dP += (size_t)b * (size_t)(a.n_psi + 1);
    return a;
}

// plasma j's record.  A pointer read from a table in memory is a flat one to the
// compiler (a kernel's own pointer arguments it knows to be global), and the loads
// through it would be flat_load where the single-plasma kernels have global_load.  So
// the record's two pointers are read as what they are, global pointers, and only then
// handed on as plain ones: the address space then follows them into the device functions.
__device__ __forceinline__ PlasmaRec plasma_rec(const PlasmaRec *plasmas, int j) {
    typedef const __attribute__((address_space(1))) double *gptr;
    const PlasmaRec *q = plasmas + j;
    gptr coef, cellp;
    __builtin_memcpy(&coef, &q->coef, sizeof(coef));
    __builtin_memcpy(&cellp, &q->cellp, sizeof(cellp));
    return PlasmaRec{(const double *)coef, (const double *)cellp, q->g, q->psi_max};
}

// beam_args with the beam's plasma in place of the handle's
__device__ __forceinline__ TraceArgs beam_args(const BeamsPlArgs &pa, int b, const BeamRec &br) {
    TraceArgs a = beam_args((const BeamsArgs &)pa, b, br);
    const PlasmaRec pr = plasma_rec(pa.plasmas, pa.beam_pl[b]);
    a.coef = pr.coef, a.cellp = pr.cellp, a.g = pr.g;
    return a;
}

// the plasma beam b goes through: the one in the kernel's own arguments, or the
// listed one the tables name
__device__ __forceinline__ PlasmaRec beam_plasma(const PlasmaRec &own, int) { return own; }
__device__ __forceinline__ PlasmaRec beam_plasma(const PlasmaRec &, int b, const PlasmaRec *plasmas,
                                                 const int *beam_pl) {
    return plasma_rec(plasmas, beam_pl[b]);
}

// grid: the wave table's entries; 64 lanes.  BA: BeamsArgs or BeamsPlArgs
template <int ABS, int DEPO, bool TRAJ, int LPR, class BA>
__global__ void __launch_bounds__(64, TORJ_MIN_WAVES) k_trace_beams(BA ba) {
    const BeamWave wv = ba.waves[blockIdx.x];
    const BeamRec br = ba.beams[wv.beam];
    const TraceArgs a = beam_args(ba, wv.beam, br);
    const int i = wv.first + (int)threadIdx.x / LPR, sub = (int)threadIdx.x % LPR;
    AlbajarWork work = {};
    unsigned long long steps = 0;
    if (i < br.hi) {
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

// k_final_alpha with the ray's beam's constants and plasma
template <int ABS, class BA>
__global__ void __launch_bounds__(64) k_final_alpha_beams(BA ba) {
    const TraceArgs &a = ba.a;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int k = a.steps[i];
    if (k <= 0) return;
    const int b = beam_of(ba.beams, ba.n_beams, i);
    const TraceArgs ab = beam_args(ba, b, ba.beams[b]);
    double x[3], N[3], du[6], al = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        x[c] = a.state[c * a.n + i];
        N[c] = a.state[(3 + c) * a.n + i];
    }
    if constexpr (ABS != 0) ray_rhs_m<ABS>(ab.coef, ab.g, ab.k, c_gl, ab.omega, ab.mode, a.abs_model, x, N, du, al, nullptr);
    a.smp_dpds[smp_at(k, i, a.smp_rows)] = exp(-a.state[6 * a.n + i]) * al;
}

// ---- ray profiles (torj_ray_profile[_device]): one row of kProfCols columns per saved point
// of a ray, prof[(row * kProfCols + c) * n + i], NaN-filled before the two kernels below ----
// Stage A, the latency chain: k_trace_beams' body without deposition.  Lane sub == 0 stores
// (x, N, tau, s) of row 0 ahead of the loop and of row steps / traj_stride where the trace
// stores a trajectory sample (ray_segment's PROF): nothing is evaluated for the table here.
// grid: the wave table's entries; 64 lanes
template <int ABS, int LPR, class BA>
__global__ void __launch_bounds__(64, TORJ_MIN_WAVES) k_profile_beams(BA ba, double *prof) {
    const BeamWave wv = ba.waves[blockIdx.x];
    const BeamRec br = ba.beams[wv.beam];
    const TraceArgs a = beam_args(ba, wv.beam, br);
    const int i = wv.first + (int)threadIdx.x / LPR, sub = (int)threadIdx.x % LPR;
    AlbajarWork work = {};
    unsigned long long steps = 0;
    if (i < br.hi) {
        RayState r;
        load_start(a, i, r);
        if (sub == 0) profile_store(prof, a, i, 0, r.x, r.N, r.tau, 0);
        ray_segment<ABS, kDepoNone, false, LPR, true>(a, i, 1.0, r, a.n_steps, work, sub, prof);
        if (sub == 0) {
            store_state(a, i, r);
            steps = r.steps;
        }
    }
    flush_counters(a, steps, 4ull * steps, work);
}

// Stage B, fully parallel: one lane per (row, ray), grid (ceil(n / 64), n_rows), the ray index
// fastest.  A row the trace did not reach keeps its NaN fill; a stored one gets columns 8-24
// from its (x, N) with the ray's beam's constants and plasma: the device functions of
// k_eval_plasma, k_dispersion<true> and k_refr.  alpha is alpha_approx as k_dispersion gives
// it (every harmonic evaluated, no tiny-alpha skip); ABS 0: alpha = 0.
// T: the ray's entry of column 0 of one row; ab: its beam's arguments
template <int ABS>
__device__ __forceinline__ void profile_row(const TraceArgs &ab, double *T, size_t n) {
    double x[3], N[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        x[c] = T[c * n];
        N[c] = T[(3 + c) * n];
    }
    if (x[0] != x[0]) return;
    PlasmaPoint p;
    plasma_point<true>(ab.coef, ab.g, ab.k, x, p);
    double du[6], Npar, inv;
    const double D = dispersion_grad(p, N, ab.mode, du, &Npar, &inv);
    const double Nabs = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
    const double Te = exp(p.lnTe);
    double al = 0.0;
    if constexpr (ABS != 0) al = abs_albajar_fast(c_gl, ab.omega, p.X, p.Y, Nabs, Npar, Te, ab.mode, nullptr);
    const double P = exp(-T[6 * n]);
    T[8 * n] = P;
    T[9 * n] = al;
    T[10 * n] = P * al;
    T[11 * n] = eval_one(ab.coef, ab.g, sqrt(x[0] * x[0] + x[1] * x[1]), x[2], F_PSI);
    T[12 * n] = p.ne;
    T[13 * n] = Te;
    T[14 * n] = p.B[0];
    T[15 * n] = p.B[1];
    T[16 * n] = p.B[2];
    T[17 * n] = p.Babs;
    T[18 * n] = p.X;
    T[19 * n] = p.Y;
    T[20 * n] = Npar;
    T[21 * n] = Nabs;
    T[22 * n] = refractive_index_sq(p.X, p.Y, Npar, ab.mode);
    T[23 * n] = D;
    T[24 * n] = 1.0 / inv;
}

template <int ABS, class BA>
__global__ void __launch_bounds__(64) k_profile_pts(BA ba, double *prof, int n_rows) {
    const TraceArgs &a = ba.a;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const size_t n = (size_t)a.n;
    const int b = beam_of(ba.beams, ba.n_beams, i);
    const TraceArgs ab = beam_args(ba, b, ba.beams[b]);
    // (rows beyond the grid's y extent of 65 535: the block's next rows)
    for (int row = blockIdx.y; row < n_rows; row += gridDim.y)
        profile_row<ABS>(ab, prof + (size_t)row * kProfCols * n + i, n);
}

// k_shell_sum per beam: grid (n_psi, n_beams), block (k, b) sums beam b's rays into
// row b of dP, each thread its rays lo + t, lo + t + 256, ... in k_shell_sum's order
// and unrolling, the same final reduction: the row k_shell_sum gives that beam alone
__global__ void __launch_bounds__(256) k_shell_sum_beams(FitArgs a, const BeamRec *beams) {
    const int k = blockIdx.x;
    const int lo = beams[blockIdx.y].lo, nb = beams[blockIdx.y].hi - lo;
    double acc = 0.0;
    constexpr int kB = 8;
    const bool shell = k < a.n_psi - 1;
    const double *row = (shell ? a.dPs + (size_t)k * a.n : a.Pray) + lo;
    const double *wr = a.w ? a.w + lo : nullptr;
    const int *kstar = a.kstar + lo;
    for (int i0 = threadIdx.x; i0 < nb; i0 += 256 * kB) {
        double v[kB], wv[kB];
        bool on[kB];
#pragma unroll
        for (int u = 0; u < kB; u++) {
            const int i = i0 + 256 * u;
            on[u] = i < nb;
            v[u] = on[u] ? row[i] : 0.0;
            wv[u] = on[u] && wr ? wr[i] : 1.0;
            if (shell && on[u]) on[u] = k > kstar[i];
        }
#pragma unroll
        for (int u = 0; u < kB; u++)
            if (on[u]) acc += wv[u] * v[u];
    }
    __shared__ double red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = (red[0] + red[1]) + (red[2] + red[3]);
        a.dP[(size_t)blockIdx.y * (size_t)(a.n_psi + 1) + (k < a.n_psi - 1 ? k : a.n_psi)] += t;
    }
}

// k_ray_entry with the ray's beam's frequency and mode (a.omega, a.mode unused) and,
// with the tables (PT: none, or plasmas and beam_pl), its plasma and that plasma's psi_prof_max
// (a.coef, a.g, a.psi_max then unused too)
template <class... PT>
__global__ void __launch_bounds__(64) k_ray_entry_beams(EntryArgs a, const BeamRec *beams, int n_beams, PT... pt) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int b = beam_of(beams, n_beams, i);
    const double omega = beams[b].omega;
    const int mode = beams[b].mode;
    const PlasmaRec pr = beam_plasma(PlasmaRec{a.coef, nullptr, a.g, a.psi_max}, b, pt...);
    const double x0[3] = {a.x0[i], a.x0[a.n + i], a.x0[2 * a.n + i]};
    const double N0[3] = {a.N0[i], a.N0[a.n + i], a.N0[2 * a.n + i]};
    double xo[3], No[3], s0;
    const int st = ray_entry_one(pr.coef, pr.g, pr.psi_max, x0, N0, omega, mode, xo, No, s0);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.xp[k * a.n + i] = xo[k];
        a.Np[k * a.n + i] = No[k];
    }
    a.s0[i] = s0;
    a.status[i] = st;
}

// k_fit_depo with psi at the launch point from the ray's beam's plasma (a.coef, a.g
// unused); the walk itself runs on the ray's samples
__global__ void __launch_bounds__(64, 2) k_fit_depo_pl(FitArgs a, const BeamRec *beams, int n_beams,
                                                       const PlasmaRec *plasmas, const int *beam_pl) {
    extern __shared__ double s_grid[];
    if (a.n_psi <= kFitGridLds) {
        for (int k = threadIdx.x; k < a.n_psi; k += 64) s_grid[k] = a.grid[k];
        __syncthreads();
        a.grid = s_grid;
    }
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const PlasmaRec pr = plasma_rec(plasmas, beam_pl[beam_of(beams, n_beams, i)]);
    const double xl[3] = {a.x_launch[i], a.x_launch[a.n + i], a.x_launch[2 * a.n + i]};
    fit_depo_ray<kOpenCache>(a, i, psi_at(pr.coef, pr.g, xl));
}

// ---- torj_make_beams: the rays that passed the ray entry closed up ahead of the trace, and the
// trace's outputs put back in launched order behind it (torj_launch.hpp beams_compact) ----
// m kept rays of n launched; idx[k] < n: the launched index of kept ray k
struct RaysGatherArgs {
    int n, m;
    const int *idx;
    const double *pos, *w, *xp, *Np, *s0;       // launched: 3 x n, n, 3 x n, 3 x n, n
    double *pos_c, *w_c, *xp_c, *Np_c, *s0_c;   // kept: the same rows of m
};

// one lane per kept ray, component-major on both sides
__global__ void __launch_bounds__(64) k_rays_gather(RaysGatherArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= a.m) return;
    const int i = a.idx[k];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        a.pos_c[c * a.m + k] = a.pos[c * a.n + i];
        a.xp_c[c * a.m + k] = a.xp[c * a.n + i];
        a.Np_c[c * a.m + k] = a.Np[c * a.n + i];
    }
    a.w_c[k] = a.w[i];
    a.s0_c[k] = a.s0[i];
}

// inv[i]: the kept index of launched ray i, or -1 where it failed entry: such a ray gets its
// entry status, 0 steps, P_dep 0 and NaN in state and in its traj columns (the bytes the
// trace's own NaN fill of traj writes)
struct RaysScatterArgs {
    int n, m, n_save;
    const int *inv, *entry_status;                       // n each
    const double *state_c, *P_dep_c, *traj_c;            // kept: 7 x m, m, n_save x 5 x m
    const int *status_c, *steps_c;                       // m each
    double *state, *P_dep, *traj;                        // launched: 7 x n, n, n_save x 5 x n
    int *status, *steps;                                 // n each
};

// grid (ceil(n / 64), 1 + samples' blocks): one lane per launched ray; blockIdx.y == 0 the
// final state, status, steps and P_dep, the others the saved samples, gridDim.y - 1 apart
__global__ void __launch_bounds__(64) k_rays_scatter(RaysScatterArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int k = a.inv[i];
    const double nan = __longlong_as_double(-1ll);
    if (blockIdx.y == 0) {
#pragma unroll
        for (int c = 0; c < 7; c++) a.state[c * a.n + i] = k >= 0 ? a.state_c[c * a.m + k] : nan;
        a.status[i] = k >= 0 ? a.status_c[k] : a.entry_status[i];
        a.steps[i] = k >= 0 ? a.steps_c[k] : 0;
        a.P_dep[i] = k >= 0 ? a.P_dep_c[k] : 0.0;
        return;
    }
    for (int j = (int)blockIdx.y - 1; j < a.n_save; j += (int)gridDim.y - 1)
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const size_t row = (size_t)j * 5 + c;
            a.traj[row * a.n + i] = k >= 0 ? a.traj_c[row * a.m + k] : nan;
        }
}
