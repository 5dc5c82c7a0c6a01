// torj_k_depo.hpp -- the reference-faithful deposition's kernels
// (torj_fitdepo.hpp): the one-pass k_fit_depo, the streamed windows
// k_depo_stream / _elim / _walk / _tail, torj_power_deposition_profile's
// kernels, the grid check and the shell sum.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include "torj_args.hpp"  // info_steps
#include "torj_fitdepo.hpp"

// ---------------------------------------------------------------------------
// Reference-faithful deposition (torj_fitdepo.hpp): one lane per ray
// ---------------------------------------------------------------------------
// boundaries up to this many are staged in LDS by k_fit_depo (32 KB per wave)
constexpr int kFitGridLds = 4096;

__global__ void __launch_bounds__(64, 2) k_fit_depo(FitArgs a) {
    // the walk's boundary lookups (cursor moves, root levels) form serial
    // dependency chains: LDS latency instead of L2 latency on each
    extern __shared__ double s_grid[];
    if (a.n_psi <= kFitGridLds) {
        for (int k = threadIdx.x; k < a.n_psi; k += 64) s_grid[k] = a.grid[k];
        __syncthreads();
        a.grid = s_grid;
    }
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const double xl[3] = {a.x_launch[i], a.x_launch[a.n + i], a.x_launch[2 * a.n + i]};
    fit_depo_ray<kOpenCache>(a, i, psi_at(a.coef, a.g, xl));
}
// the streamed deposition (torj_fitdepo.hpp): windows of the walk behind the
// split pipeline's scan (S = the scan's steps of a still-running ray), then the
// rest of every ray after the trace
__device__ __forceinline__ bool fit_grid_lds(FitArgs &a) {
    extern __shared__ double s_grid[];
    if (a.n_psi > kFitGridLds) return false;
    for (int k = threadIdx.x; k < a.n_psi; k += 64) s_grid[k] = a.grid[k];
    __syncthreads();
    a.grid = s_grid;
    return true;
}
// The windows' gate: a ray still running (a stopped one is k_depo_tail's),
// S = its scanned steps capped at s_cap, a new window ready; psi at the launch
// point (point 0) only for the walk's start.  s_cap: the steps whose samples
// this launch may read (the end of the block whose scan it follows).  On its
// own stream (TORJ_DEPO_STREAM=2) the launch can overlap the next block's
// scan, so sinfo may already hold that scan's carry, whose samples need not
// be visible yet: S is capped at the block end (and a ray that scan stopped is
// left to k_depo_tail).  Windows are schedule-independent (torj_fitdepo.hpp),
// so the outputs do not depend on which carry the read saw.
__device__ __forceinline__ bool depo_stream_gate(const FitArgs &a, const DepoStream &ds, const int *sinfo,
                                                 int s_cap, int i, int &S, double &psiL) {
    const int v = __hip_atomic_load(sinfo + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (info_status(v) != ST_OK) return false;
    S = min(info_steps(v), s_cap);
    const int j = ds.v[kDsJ * (size_t)a.n + i];
    if ((j < 0 ? 0 : j) + kDepoQ + 3 + kDepoW > S) return false;  // no new window yet
    psiL = 0.0;
    if (j < 0) {
        const double xl[3] = {a.x_launch[i], a.x_launch[a.n + i], a.x_launch[2 * a.n + i]};
        psiL = psi_at(a.coef, a.g, xl);
    }
    return true;
}
__global__ void __launch_bounds__(64, 2) k_depo_stream(FitArgs a, DepoStream ds, const int *sinfo, int s_cap) {
    fit_grid_lds(a);
    const int i = blockIdx.x * 64 + threadIdx.x;
    int S;
    double psiL;
    if (i >= a.n || !depo_stream_gate(a, ds, sinfo, s_cap, i, S, psiL)) return;
    fit_depo_stream(a, ds, i, psiL, S);
}
// TORJ_DEPO_STREAM=3: a window's elimination and walk as two launches
// (torj_fitdepo.hpp fit_depo_stream_elim / _walk), the same S and gating
#ifndef TORJ_DEPO_ELIM_WAVES
#define TORJ_DEPO_ELIM_WAVES 4
#endif
__global__ void __launch_bounds__(64, TORJ_DEPO_ELIM_WAVES) k_depo_elim(FitArgs a, DepoStream ds, const int *sinfo,
                                                                        int s_cap) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    int S;
    double psiL;
    if (i >= a.n || !depo_stream_gate(a, ds, sinfo, s_cap, i, S, psiL)) return;
    fit_depo_stream_elim(a, ds, i, psiL, S);
}
#ifndef TORJ_DEPO_WALK_WAVES
#define TORJ_DEPO_WALK_WAVES 3  // 168 VGPRs at kWalkChunkStream = 1, no spill
#endif
__global__ void __launch_bounds__(64, TORJ_DEPO_WALK_WAVES) k_depo_walk(FitArgs a, DepoStream ds, const int *sinfo,
                                                                        int s_cap) {
    fit_grid_lds(a);
    const int i = blockIdx.x * 64 + threadIdx.x;
    int S;
    double psiL;
    if (i >= a.n || !depo_stream_gate(a, ds, sinfo, s_cap, i, S, psiL)) return;
    fit_depo_stream_walk(a, ds, i, psiL, S);
}
__global__ void __launch_bounds__(64, 2) k_depo_tail(FitArgs a, DepoStream ds) {
    fit_grid_lds(a);
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const double xl[3] = {a.x_launch[i], a.x_launch[a.n + i], a.x_launch[2 * a.n + i]};
    fit_depo_tail(a, ds, i, psi_at(a.coef, a.g, xl));
}
// torj_power_deposition_profile: the caller's vectors of ray i (points off[i] ..
// off[i] + npts[i] - 1) into the fit's per-point rows, psi(s_j) from the psi
// spline at x_j (src/plasma.jl:95-98: psi_norm_spline(hypot(x, y), z))
__global__ void __launch_bounds__(64) k_profile_samples(FitArgs a, const long *off, const double *s,
                                                        const double *x, size_t n_all, const double *dpds) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    for (int j = 0; j < a.npts[i]; j++) {
        const size_t q = (size_t)off[i] + j;
        const double xq[3] = {x[q], x[n_all + q], x[2 * n_all + q]};
        const size_t o = smp_at(j, i, a.rows);
        // (FitArgs holds the sample rows read-only for the fit; this kernel fills them)
        const_cast<double *>(a.smp_psi)[o] = psi_at(a.coef, a.g, xq);
        const_cast<double *>(a.smp_dpds)[o] = dpds[q];
        const_cast<double *>(a.smp_s)[o] = s[q];
    }
}
__global__ void __launch_bounds__(64, 2) k_fit_profile(FitArgs a) {
    extern __shared__ double s_grid[];
    if (a.n_psi <= kFitGridLds) {
        for (int k = threadIdx.x; k < a.n_psi; k += 64) s_grid[k] = a.grid[k];
        __syncthreads();
        a.grid = s_grid;
    }
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    fit_depo_ray<kOpenCache>(a, i, 0.0);
}
// psi_dP_dV strictly increasing (the shell lookups assume it)
__global__ void __launch_bounds__(256) k_grid_check(const double *grid, int n, int *flags) {
    bool bad = false;
    for (int k = threadIdx.x + 1; k < n; k += 256) bad |= !(grid[k] > grid[k - 1]);
    if (bad) atomicOr(flags, 1);
}

__global__ void __launch_bounds__(256) k_shell_sum(FitArgs a) {
    const int k = blockIdx.x;
    double acc = 0.0;
    // each thread's rays i, i + 256, ... in order, their loads eight at a time
    // (one memory latency per eight rays instead of one per ray; the same sum)
    constexpr int kB = 8;
    const bool shell = k < a.n_psi - 1;
    const double *row = shell ? a.dPs + (size_t)k * a.n : a.Pray;
    for (int i0 = threadIdx.x; i0 < a.n; i0 += 256 * kB) {
        double v[kB], wv[kB];
        bool on[kB];
#pragma unroll
        for (int u = 0; u < kB; u++) {
            const int i = i0 + 256 * u;
            on[u] = i < a.n;
            v[u] = on[u] ? row[i] : 0.0;
            wv[u] = on[u] && a.w ? a.w[i] : 1.0;
            if (shell && on[u]) on[u] = k > a.kstar[i];
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
        a.dP[k < a.n_psi - 1 ? k : a.n_psi] += t;
    }
}

