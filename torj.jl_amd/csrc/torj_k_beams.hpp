// torj_k_beams.hpp -- the multi-beam forms of the one-shot trace and of the
// kernels around it: B beams' rays concatenated, each beam with its own
// frequency and mode and its own row of dP_shell (BeamsArgs, torj_args.hpp; the
// tables come from torj_launch.hpp beams_plan).  k_trace_beams runs one wave per
// workgroup, wave w the rays its table entry names: the lanes of a wave are
// k_trace's on that beam alone, and the beam's omega, Consts and mode are
// uniform over the wave (scalar loads by blockIdx, SGPRs as k_trace's kernel
// arguments are).  The device functions are k_trace's, unchanged.
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

// grid: the wave table's entries; 64 lanes
template <int ABS, int DEPO, bool TRAJ, int LPR = 1>
__global__ void __launch_bounds__(64, TORJ_MIN_WAVES) k_trace_beams(BeamsArgs ba) {
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

// k_final_alpha with the ray's beam's constants
template <int ABS>
__global__ void __launch_bounds__(64) k_final_alpha_beams(BeamsArgs ba) {
    const TraceArgs &a = ba.a;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int k = a.steps[i];
    if (k <= 0) return;
    const BeamRec br = ba.beams[beam_of(ba.beams, ba.n_beams, i)];
    double x[3], N[3], du[6], al = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        x[c] = a.state[c * a.n + i];
        N[c] = a.state[(3 + c) * a.n + i];
    }
    if constexpr (ABS != 0) ray_rhs_m<ABS>(a.coef, a.g, br.k, c_gl, br.omega, br.mode, a.abs_model, x, N, du, al, nullptr);
    a.smp_dpds[smp_at(k, i, a.smp_rows)] = exp(-a.state[6 * a.n + i]) * al;
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

// k_ray_entry with the ray's beam's frequency and mode (a.omega, a.mode unused)
__global__ void __launch_bounds__(64) k_ray_entry_beams(EntryArgs a, const BeamRec *beams, int n_beams) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int b = beam_of(beams, n_beams, i);
    const double omega = beams[b].omega;
    const int mode = beams[b].mode;
    const double x0[3] = {a.x0[i], a.x0[a.n + i], a.x0[2 * a.n + i]};
    const double N0[3] = {a.N0[i], a.N0[a.n + i], a.N0[2 * a.n + i]};
    double xo[3], No[3], s0;
    const int st = ray_entry_one(a.coef, a.g, a.psi_max, x0, N0, omega, mode, xo, No, s0);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.xp[k * a.n + i] = xo[k];
        a.Np[k * a.n + i] = No[k];
    }
    a.s0[i] = s0;
    a.status[i] = st;
}
