// torj_k_beams_pl.hpp -- torj_k_beams.hpp's kernels for beams that go through
// differing plasmas (BeamsPlArgs, torj_args.hpp; the tables come from
// torj_launch.hpp beams_plasmas_plan): beam b is traced through the listed plasma
// beam_pl[b], whose coefficients, cell table and grid replace the handle's in the
// trace's arguments.  A wave never mixes beams, so its plasma is wave-uniform like
// its omega: k_trace_beams_pl loads the record by blockIdx (scalar loads, SGPRs).
// The kernels after the trace run one lane per ray and look the ray's beam up, then
// that beam's plasma.  The device functions are k_trace's, unchanged; each kernel
// is its torj_k_beams.hpp twin plus the plasma record.
// (a slice of torj_hip.hip: included after `using namespace torj`)
#pragma once
#include "torj_k_beams.hpp"

// plasma j's record.  A pointer read from a table in memory is a flat one to the
// compiler (a kernel's own pointer arguments it knows to be global), and the loads
// through it would be flat_load where the twins have global_load.  So the record's two
// pointers are read as what they are, global pointers, and only then handed on as
// plain ones: the address space then follows them into the device functions.
__device__ __forceinline__ PlasmaRec plasma_rec(const PlasmaRec *plasmas, int j) {
    typedef const __attribute__((address_space(1))) double *gptr;
    const PlasmaRec *q = plasmas + j;
    gptr coef, cellp;
    __builtin_memcpy(&coef, &q->coef, sizeof(coef));
    __builtin_memcpy(&cellp, &q->cellp, sizeof(cellp));
    return PlasmaRec{(const double *)coef, (const double *)cellp, q->g, q->psi_max};
}

// beam_args with the beam's plasma in place of the handle's
__device__ __forceinline__ TraceArgs beam_pl_args(const BeamsPlArgs &pa, int b, const BeamRec &br) {
    TraceArgs a = beam_args(pa.b, b, br);
    const PlasmaRec pr = plasma_rec(pa.plasmas, pa.beam_pl[b]);
    a.coef = pr.coef, a.cellp = pr.cellp, a.g = pr.g;
    return a;
}

// grid: the wave table's entries; 64 lanes
template <int ABS, int DEPO, bool TRAJ, int LPR = 1>
__global__ void __launch_bounds__(64, TORJ_MIN_WAVES) k_trace_beams_pl(BeamsPlArgs pa) {
    const BeamWave wv = pa.b.waves[blockIdx.x];
    const BeamRec br = pa.b.beams[wv.beam];
    const TraceArgs a = beam_pl_args(pa, wv.beam, br);
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

// k_final_alpha_beams with the ray's beam's plasma
template <int ABS>
__global__ void __launch_bounds__(64) k_final_alpha_beams_pl(BeamsPlArgs pa) {
    const TraceArgs &a = pa.b.a;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int k = a.steps[i];
    if (k <= 0) return;
    const int b = beam_of(pa.b.beams, pa.b.n_beams, i);
    const BeamRec br = pa.b.beams[b];
    const PlasmaRec pr = plasma_rec(pa.plasmas, pa.beam_pl[b]);
    double x[3], N[3], du[6], al = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        x[c] = a.state[c * a.n + i];
        N[c] = a.state[(3 + c) * a.n + i];
    }
    if constexpr (ABS != 0) ray_rhs_m<ABS>(pr.coef, pr.g, br.k, c_gl, br.omega, br.mode, a.abs_model, x, N, du, al, nullptr);
    a.smp_dpds[smp_at(k, i, a.smp_rows)] = exp(-a.state[6 * a.n + i]) * al;
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

// k_ray_entry_beams with the ray's beam's plasma and its psi_prof_max (a.coef, a.g,
// a.psi_max unused)
__global__ void __launch_bounds__(64) k_ray_entry_beams_pl(EntryArgs a, const BeamRec *beams, int n_beams,
                                                           const PlasmaRec *plasmas, const int *beam_pl) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int b = beam_of(beams, n_beams, i);
    const double omega = beams[b].omega;
    const int mode = beams[b].mode;
    const PlasmaRec pr = plasma_rec(plasmas, beam_pl[b]);
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
