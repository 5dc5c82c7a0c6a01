// torj_k_points.hpp -- the kernels that evaluate at given points, outside the
// trace: the GPU ray entry, dP/ds at a ray's last point, and the batched
// plasma / dispersion / absorption / refractive-index evaluations.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include "torj_args.hpp"
#include "torj_entry.hpp"
#include "torj_k_fused.hpp"  // c_gl
#include "torj_warm.hpp"

// ---------------------------------------------------------------------------
// GPU ray entry (src/solve.jl:7-74): one lane per ray.  The bisection to the
// psi_prof_max surface runs ~55 spline evaluations per lane; lanes of a wave
// take nearly the same number, so 64-lane blocks keep divergence low.
// ---------------------------------------------------------------------------
struct EntryArgs {
    const double *coef;
    Grid g;
    double psi_max, omega;
    int mode, n;
    const double *x0, *N0;
    double *xp, *Np, *s0;
    int *status;
};

__global__ void __launch_bounds__(64) k_ray_entry(EntryArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const double x0[3] = {a.x0[i], a.x0[a.n + i], a.x0[2 * a.n + i]};
    const double N0[3] = {a.N0[i], a.N0[a.n + i], a.N0[2 * a.n + i]};
    double xo[3], No[3], s0;
    const int st = ray_entry_one(a.coef, a.g, a.psi_max, x0, N0, a.omega, a.mode, xo, No, s0);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.xp[k * a.n + i] = xo[k];
        a.Np[k * a.n + i] = No[k];
    }
    a.s0[i] = s0;
    a.status[i] = st;
}

// dP/ds at a ray's last saved point (every other point's alpha is the next
// step's stage-0 RHS inside the trace kernel): P alpha_approx(x, N) from the
// final state (src/solve.jl:171)
template <int ABS>
__global__ void __launch_bounds__(64) k_final_alpha(TraceArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int k = a.steps[i];
    if (k <= 0) return;
    double x[3], N[3], du[6], al = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        x[c] = a.state[c * a.n + i];
        N[c] = a.state[(3 + c) * a.n + i];
    }
    if constexpr (ABS != 0) ray_rhs_m<ABS>(a.coef, a.g, a.k, c_gl, a.omega, a.mode, a.abs_model, x, N, du, al, nullptr);
    a.smp_dpds[smp_at(k, i, a.smp_rows)] = exp(-a.state[6 * a.n + i]) * al;
}

struct EvalArgs {
    const double *coef;
    Grid g;
    Consts k;
    double omega;
    int mode;
    int n;
    const double *x, *N;
    double *out;
    double *D, *du, *alpha;
};

__global__ void __launch_bounds__(256, 1) k_eval_plasma(EvalArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double x[3], N[3];
    for (int c = 0; c < 3; c++) {
        x[c] = a.x[c * a.n + i];
        N[c] = a.N[c * a.n + i];
    }
    PlasmaPoint p;
    plasma_point<true>(a.coef, a.g, a.k, x, p);
    const double R = sqrt(x[0] * x[0] + x[1] * x[1]);
    double *o = a.out;
    const size_t n = a.n;
    o[0 * n + i] = p.B[0];
    o[1 * n + i] = p.B[1];
    o[2 * n + i] = p.B[2];
    o[3 * n + i] = p.ne;
    o[4 * n + i] = exp(p.lnTe);
    o[5 * n + i] = eval_one(a.coef, a.g, R, x[2], F_PSI);
    o[6 * n + i] = p.X;
    o[7 * n + i] = p.Y;
    o[8 * n + i] = N[0] * p.b[0] + N[1] * p.b[1] + N[2] * p.b[2];
    o[9 * n + i] = p.b[0];
    o[10 * n + i] = p.b[1];
    o[11 * n + i] = p.b[2];
    o[12 * n + i] = p.Babs;
}

template <bool ABS>
__global__ void __launch_bounds__(256, 1) k_dispersion(EvalArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double x[3], N[3], du[6], alpha;
    for (int c = 0; c < 3; c++) {
        x[c] = a.x[c * a.n + i];
        N[c] = a.N[c * a.n + i];
    }
    PlasmaPoint p;
    plasma_point<ABS>(a.coef, a.g, a.k, x, p);
    double Npar;
    const double D = dispersion_grad(p, N, a.mode, du, &Npar);
    if (a.D) a.D[i] = D;
    if (a.du)
        for (int c = 0; c < 6; c++) a.du[c * a.n + i] = du[c];
    if constexpr (ABS) {
        const double Nabs = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
        alpha = abs_albajar_fast(c_gl, a.omega, p.X, p.Y, Nabs, Npar, exp(p.lnTe), a.mode, nullptr);
        a.alpha[i] = alpha;
    }
}

struct AlbArgs {
    int n, mode;
    const double *omega, *X, *Y, *Nabs, *Npar, *Te;
    double *out;
    const double *inv;  // warm: 1 / |dD/dN|
    double *n2;         // warm: N_perp^2 (re, im interleaved), may be null
    int iwarm;
};

// warm absorption alpha (torj_warm.hpp) at arbitrary points: one lane each
__global__ void __launch_bounds__(64) k_alpha_warm(AlbArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    cplx n2;
    a.out[i] = alpha_warm(a.omega[i], a.X[i], a.Y[i], a.Nabs[i], a.Npar[i], a.Te[i], a.inv[i],
                          a.mode, a.iwarm, &n2);
    if (a.n2) {
        a.n2[2 * i] = n2.re;
        a.n2[2 * i + 1] = n2.im;
    }
}

__global__ void __launch_bounds__(256, 1) k_albajar(AlbArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    a.out[i] = abs_albajar_fast(c_gl, a.omega[i], a.X[i], a.Y[i], a.Nabs[i], a.Npar[i], a.Te[i],
                                a.mode, nullptr);
}

__global__ void k_refr(AlbArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    a.out[i] = refractive_index_sq(a.X[i], a.Y[i], a.Npar[i], a.mode);
}

