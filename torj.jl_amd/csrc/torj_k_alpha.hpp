// torj_k_alpha.hpp -- the split pipeline's alpha kernels at the stored stage
// points: k_alpha_pts (Albajar; k_alpha_pts_mp, several points per wave) and
// the warm k_alpha_warm_pts / k_alpha_warm_big with their deferred list.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include "torj_args.hpp"
#include "torj_k_fused.hpp"  // c_gl
#include "torj_warm.hpp"

// alpha at the stored stage points of one block: block = kAlphaBlock lanes
// (TORJ_ALPHA_BLOCK, default 128: two groups of 64 rays) at one (step j,
// stage); lanes of rays the trajectory did not
// reach this step with (or the scan has stopped) sit out, as in the fused wave
// (a measured alternative -- harmonic 2 in a second pass over a compacted list
// of the points needing it -- executed more instructions in total: the points
// needing harmonic 2 cluster in whole waves)
// COUNT: a counted launch (sp.awork set) -- the work words are written; an
// uncounted one carries no work struct at all (with its address taken
// conditionally it lived in scratch: 32 B of stores per lane and point, ~25 GB
// per headline launch)
#ifndef TORJ_ALPHA_BLOCK
#define TORJ_ALPHA_BLOCK 128  // lanes per alpha workgroup (groups of 64 rays at one (step, stage)): two
// waves, placed beside the trajectory waves SIMD pair by SIMD pair (256: 47.4-47.8 ms
// trace phase, 128: 45.6-45.7, 64: 46.7-48.6 alternating)
#endif
constexpr int kAlphaBlock = TORJ_ALPHA_BLOCK;
static_assert(kAlphaBlock % 64 == 0, "an alpha wave holds one 64-ray group");
// The head of an alpha wave (round 13).  Before: five dependent round trips
// ahead of the first fp64 instruction -- a.n; the tinfo / sinfo / zflag
// pointers; ti, si and the flag byte, waited for because the wave's exit hangs on
// the byte; the ain / alpha pointers and nf; the five inputs.  Now: the kernel
// arguments in one scalar batch (alpha_args_batch), the group's flag word as one
// scalar load (alpha_group_flagged), and for a wave that evaluates, ti, si and
// the five inputs as one vector batch behind a single wait.
//
// every kernel argument the head needs, consumed by an empty asm so that the
// compiler loads them together at the top instead of each before its first use
#if defined(__HIP_DEVICE_COMPILE__)
#define TORJ_ALPHA_ARGS_BATCH(a, sp)                                                                        \
    asm volatile("" ::"s"((a).n), "s"((sp).gflag), "s"((sp).zflag), "s"((sp).tinfo), "s"((sp).sinfo),      \
                 "s"((sp).ain), "s"((sp).alpha), "s"((sp).nf), "s"((sp).k0))
#else
#define TORJ_ALPHA_ARGS_BATCH(a, sp) \
    do {                             \
    } while (0)
#endif
// The word of the wave's 64-ray group (SplitArgs::gflag; w0: the wave's first
// ray, wave-uniform and < n).  Uniform address, so a scalar load, and a scalar
// load is safe here: the word was written by the trajectory kernel of this
// block, which finished before this kernel was launched (the stream event
// between them), and it sits in a 256-byte-aligned array of its ring slot alone,
// which no kernel running beside this one writes -- the trajectory kernels ahead
// write other slots' arrays, never this line, until this block's scan is done.
// So the scalar cache, which is not coherent with vector stores, cannot hold an
// older copy than the launch's own invalidate leaves it.
__device__ __forceinline__ bool alpha_group_flagged(const SplitArgs &sp, int w0) {
    return sp.gflag != nullptr && group_word(sp.gflag, w0 >> 6) != 0u;
}
#ifndef TORJ_ALPHA_SETPRIO
#define TORJ_ALPHA_SETPRIO 0
#endif
template <bool COUNT>
__global__ void __launch_bounds__(kAlphaBlock, TORJ_ALPHA_WAVES) k_alpha_pts(TraceArgs a, SplitArgs sp, int nq) {
#if TORJ_ALPHA_SETPRIO
    __builtin_amdgcn_s_setprio(TORJ_ALPHA_SETPRIO);  // measurement knob: the alpha waves' issue priority
#endif
    const int q = blockIdx.x, js = blockIdx.y;  // js = j * 4 + stage (a 2-D grid: no division)
    const int i = q * kAlphaBlock + threadIdx.x;
    TORJ_ALPHA_ARGS_BATCH(a, sp);
    const int w0 = __builtin_amdgcn_readfirstlane(i & ~63);  // the wave's first ray
    if (w0 >= a.n) return;  // a whole wave past the last ray (it has no group word)
    // a group whose rays all carry the trajectory kernel's block zero flag
    // (abs_albajar_fast_body's early settle returns +0 at every point of theirs):
    // the wave ends here, with no vector load and no store -- the scan reads the
    // same word and takes sp.zval for the group's alphas, 0 for its work words
    // (39 % of the headline beam's waves; round 6 ended them behind one vector
    // round trip and 512 B of zeros each)
    if (alpha_group_flagged(sp, w0)) {
#if defined(TORJ_ALPHA_PROF) && defined(__HIP_DEVICE_COMPILE__)
        TORJ_APROF_WAVE(kAprofZ);
#endif
        return;
    }
    if (i >= a.n) return;
    const int j = js >> 2;
    // the stop words and the five inputs at once (one memory latency; the
    // addresses are valid for any i < n whether or not the point is live).  The
    // per-ray flag byte rides with them only where it is looked at: without
    // group words (TORJ_ALPHA_GFLAG=0), or for the TORJ_ALPHA_PROF census
#if defined(TORJ_ALPHA_PROF)
    const bool want_zf = sp.zflag != nullptr;
#else
    const bool want_zf = sp.zflag != nullptr && sp.gflag == nullptr;
#endif
    const int ti = sp.tinfo[i], si = sp.sinfo[i];
    const int zf = want_zf ? sp.zflag[i] : 0;
    const double *in = sp.ain + (size_t)js * sp.nf * a.n + i;
    const double X = in[0], Y = in[(size_t)a.n], N2 = in[2 * (size_t)a.n], Npar = in[3 * (size_t)a.n];
    const double lnTe = in[4 * (size_t)a.n];
    // (an empty asm that consumes them: the compiler would otherwise sink the
    // input loads below the stop test and the Te test, three latencies in a row)
    asm volatile("" ::"v"(ti), "v"(si), "v"(zf), "v"(X), "v"(Y), "v"(N2), "v"(Npar), "v"(lnTe));
    // without group words: a wave whose rays all carry the flag writes the zeros
    // itself, as since round 6 (now behind the one batch, inputs included).  Both
    // ballots here, while zf is in hand: taken at the store, the second one kept zf
    // alive across the head and cost the kernel two VGPRs (77 -> 79)
    const bool per_ray = sp.gflag == nullptr;
    const unsigned long long zb0 = per_ray ? __ballot(zf == 0) : 1ull, zb2 = per_ray ? __ballot(zf == 2) : 0ull;
    if (zb0 == 0ull) {
#if defined(TORJ_ALPHA_PROF) && defined(__HIP_DEVICE_COMPILE__)
        TORJ_APROF_WAVE(kAprofZ);
#endif
        // (all bytes 1: the exact-zero proof, sp.zval; some 2: the tiny_alpha proof, sp.tval)
        sp.alpha[(size_t)js * a.n + i] = zb2 == 0ull ? sp.zval : sp.tval;
        if constexpr (COUNT) sp.awork[(size_t)js * a.n + i] = 0u;
        return;
    }
    // sinfo may be stale (k_tau_scan of an earlier block runs on another
    // stream): an optimisation only, as in traj_body -- a stale OK evaluates an
    // alpha the scan never reads
    if (sp.k0 + j >= info_steps(ti) || info_status(si) != ST_OK) return;
#if defined(TORJ_ALPHA_PROF) && defined(__HIP_DEVICE_COMPILE__)
    {
        // [14]: the live lanes of these (not fully flagged) waves that carry a
        // zero flag -- what compacting the unflagged points into full waves would save
        const unsigned long long am = __ballot(1), zm = __ballot(zf != 0);
        if ((int)__lane_id() == __builtin_ffsll((long long)am) - 1) {
            atomicAdd(&g_aprof[4], 1ull);
            atomicAdd(&g_aprof[5], (unsigned long long)__popcll(am));
            atomicAdd(&g_aprof[14], (unsigned long long)__popcll(zm));
        }
    }
#endif
    const double Nabs = TORJ_AIN_TRAJ_MATH ? N2 : sqrt_pos(N2), Te = TORJ_AIN_TRAJ_MATH ? lnTe : exp_fast<true>(lnTe);
    if constexpr (COUNT) {
        AlbajarWork work = {};
        sp.alpha[(size_t)js * a.n + i] = abs_albajar_fast_body<1, TORJ_ALPHA_UNROLL>(
            c_gl, a.omega, X, Y, Nabs, Npar, Te, a.mode, &work, 0, c_gl.tiny_alpha);
        sp.awork[(size_t)js * a.n + i] = (work.n_active & 1u) | ((work.n_harm & 3u) << 1) |
                                     ((work.n_zero & 3u) << 3) | (min(work.n_terms, 2047u) << 5) |
                                     ((work.n_negl & 3u) << 16) | ((work.n_early & 3u) << 18);
    } else {
        sp.alpha[(size_t)js * a.n + i] = abs_albajar_fast_body<1, TORJ_ALPHA_UNROLL>(
            c_gl, a.omega, X, Y, Nabs, Npar, Te, a.mode, nullptr, 0, c_gl.tiny_alpha);
    }
}

// k_alpha_pts with each workgroup taking P consecutive (step, stage) points of
// its rays (TORJ_ALPHA_PPW = P > 1, a measurement variant): the kernel's per-wave
// setup (arguments, the 2-D index, the rays' stop words) once per P points, and
// the next point's five inputs loaded while the current one is evaluated.  The
// lanes of a wave at one point are the same rays as k_alpha_pts' wave there, so
// the Bessel-level ballot and every alpha are the same bits.
#ifndef TORJ_ALPHA_PPW
#define TORJ_ALPHA_PPW 1
#endif
#ifndef TORJ_ALPHA_PREFETCH
#define TORJ_ALPHA_PREFETCH 1
#endif
template <bool COUNT, int P>
__global__ void __launch_bounds__(kAlphaBlock, TORJ_ALPHA_WAVES) k_alpha_pts_mp(TraceArgs a, SplitArgs sp, int nq) {
    const int i = blockIdx.x * kAlphaBlock + threadIdx.x;
    TORJ_ALPHA_ARGS_BATCH(a, sp);
    const int w0 = __builtin_amdgcn_readfirstlane(i & ~63);  // the wave's first ray
    if (w0 >= a.n) return;
    // a flagged group (as k_alpha_pts): none of the block's points is evaluated or stored
    if (alpha_group_flagged(sp, w0)) return;
    if (i >= a.n) return;
    const int js0 = blockIdx.y * P;
    const int np = min(P, 4 * sp.kb - js0);  // workgroup-uniform
    const int ti = sp.tinfo[i], si = sp.sinfo[i];
    // the ray's last stored point + 1 (0 when the scan has stopped it: sinfo may
    // be stale, an optimisation only, as in k_alpha_pts)
    const int js_end = info_status(si) != ST_OK ? 0 : 4 * (info_steps(ti) - sp.k0);
    const size_t n = (size_t)a.n, stride = (size_t)sp.nf * n;
    const double *in = sp.ain + (size_t)js0 * stride + i;
    double X = in[0], Y = in[n], N2 = in[2 * n], Npar = in[3 * n], lnTe = in[4 * n];
    for (int p = 0; p < np; p++) {
        const int js = js0 + p;
        // the quadrature table's address laundered per point: its loads (and the
        // address arithmetic) stay inside the loop instead of being hoisted into
        // registers live across the whole body (hundreds of SGPR spills otherwise)
        const GLTable *glp = &c_gl;
        asm volatile("" : "+s"(glp));
#if TORJ_ALPHA_PREFETCH
        double Xn = 0.0, Yn = 0.0, N2n = 0.0, Nparn = 0.0, lnTen = 0.0;
        if (p + 1 < np) {  // the next point's inputs in flight during this one
            const double *nx = in + (size_t)(p + 1) * stride;
            Xn = nx[0], Yn = nx[n], N2n = nx[2 * n], Nparn = nx[3 * n], lnTen = nx[4 * n];
        }
#endif
        if (js < js_end) {
            const double Nabs = TORJ_AIN_TRAJ_MATH ? N2 : sqrt_pos(N2),
                         Te = TORJ_AIN_TRAJ_MATH ? lnTe : exp_fast<true>(lnTe);
            if constexpr (COUNT) {
                AlbajarWork work = {};
                sp.alpha[(size_t)js * n + i] = abs_albajar_fast_body<1, TORJ_ALPHA_UNROLL>(
                    *glp, a.omega, X, Y, Nabs, Npar, Te, a.mode, &work, 0, glp->tiny_alpha);
                sp.awork[(size_t)js * n + i] = (work.n_active & 1u) | ((work.n_harm & 3u) << 1) |
                                               ((work.n_zero & 3u) << 3) | (min(work.n_terms, 2047u) << 5) |
                                               ((work.n_negl & 3u) << 16) | ((work.n_early & 3u) << 18);
            } else {
                sp.alpha[(size_t)js * n + i] = abs_albajar_fast_body<1, TORJ_ALPHA_UNROLL>(
                    *glp, a.omega, X, Y, Nabs, Npar, Te, a.mode, nullptr, 0, glp->tiny_alpha);
            }
        }
#if TORJ_ALPHA_PREFETCH
        X = Xn, Y = Yn, N2 = N2n, Npar = Nparn, lnTe = lnTen;
#else
        if (p + 1 < np) {
            const double *nx = in + (size_t)(p + 1) * stride;
            X = nx[0], Y = nx[n], N2 = nx[2 * n], Npar = nx[3 * n], lnTe = nx[4 * n];
        }
#endif
    }
}

// the warm alpha (absorption 2 / 3, iwarm 1 / 3) at the stored stage points:
// the same points and lanes as k_alpha_pts, with the group-velocity factor
// stored by the trajectory kernel as the sixth input.  Without a ray's state
// and step chain the heavy warm code has the registers to itself
// (waves per SIMD: iwarm 1 two -- 221 ms fused, 235 at one wave, 166 at two on
// the C5 beam; iwarm 3 one -- 20.4 s, 22.2 s at two).
#ifndef TORJ_WARM1_ALPHA_WAVES
#define TORJ_WARM1_ALPHA_WAVES 2
#endif
#ifndef TORJ_WARM3_ALPHA_WAVES
#define TORJ_WARM3_ALPHA_WAVES 1
#endif
#ifndef TORJ_ALPHA_WARM_BLOCK
#define TORJ_ALPHA_WARM_BLOCK 64  // lanes per warm-alpha workgroup (C5: 139.3 ms against 142.6-143.2
// at 128 and 149.0 at 256, alternating)
#endif
constexpr int kAlphaWarmBlock = TORJ_ALPHA_WARM_BLOCK;
// COUNT: a counted launch (sp.awork set) stores the work word; without it the
// trip counts are dead and the compiler drops their arithmetic
template <bool COUNT>
__device__ __forceinline__ void warm_store(const SplitArgs &sp, int js, int i, int n, const WarmAlpha &r) {
    sp.alpha[(size_t)js * n + i] = r.alpha;
    if constexpr (COUNT)
        sp.awork[(size_t)js * n + i] = (unsigned)min(r.nasym, 127) | ((unsigned)min(r.nfad, 127) << 7) |
                                   ((unsigned)min(r.passes, 127) << 14) | ((unsigned)r.lrm << 21);
}
template <int IWARM, bool COUNT>
__global__ void __launch_bounds__(kAlphaWarmBlock, IWARM == 1 ? TORJ_WARM1_ALPHA_WAVES : TORJ_WARM3_ALPHA_WAVES)
    k_alpha_warm_pts(TraceArgs a, SplitArgs sp, int nq) {
    const int q = blockIdx.x, js = blockIdx.y;  // js = j * 4 + stage
    const int i = q * kAlphaWarmBlock + threadIdx.x;
    if (i >= a.n) return;
    const int j = js >> 2;
    // every load of the point at once (as k_alpha_pts)
    const int ti = sp.tinfo[i], si = sp.sinfo[i];
    const double *in = sp.ain + (size_t)js * kAinFW * a.n + i;
    const double X = in[0], Y = in[(size_t)a.n], Nabs = in[2 * (size_t)a.n], Npar = in[3 * (size_t)a.n];
    const double Te = in[4 * (size_t)a.n], inv = in[5 * (size_t)a.n];
    asm volatile("" ::"v"(ti), "v"(si), "v"(X), "v"(Y), "v"(Nabs), "v"(Npar), "v"(Te), "v"(inv));
    if (sp.k0 + j >= info_steps(ti) || info_status(si) != ST_OK) return;
#if defined(TORJ_WARM_PROF) && defined(__HIP_DEVICE_COMPILE__)
    static_assert(kAlphaWarmBlock == 64, "region timers: one wave per workgroup");
    wprof_init();
#endif
    const WarmSetup w = warm_setup(Y, Nabs, Npar, Te);
    // a point with lrm > 3 (~0.1 % of the C5 beam's) goes to k_alpha_warm_big:
    // this kernel then holds the lrm <= 3 tensor only (its registers, and so
    // the waves per SIMD, are sized for that), and no wave runs the lrm <= 5
    // code for all its lanes because one of them needs it
    const bool big = w.lrm > sp.defer_lrm;
    const unsigned long long bmask = __ballot(big);
    if (bmask) {  // wave-aggregated append
        const int lane = (int)__lane_id(), lead = __builtin_ffsll((long long)bmask) - 1;
        unsigned base = 0;
        if (lane == lead) base = atomicAdd(sp.defer_cnt, (unsigned)__popcll(bmask));
        base = __shfl(base, lead);
        if (big)
            sp.defer[base + __popcll(bmask & ((1ull << lane) - 1))] =
                ((unsigned long long)js << 32) | (unsigned)i;
    }
    if (big) return;
    const WarmAlpha r = alpha_warm_l<IWARM, 3>(a.omega, X, Y, Npar, w, inv, a.mode);
    warm_store<COUNT>(sp, js, i, a.n, r);
#if defined(TORJ_WARM_PROF) && defined(__HIP_DEVICE_COMPILE__)
    TORJ_WPROF(6);  // the stores
    wprof_flush();
#endif
}

// the points k_alpha_warm_pts deferred (lrm > 3), with the lrm <= 5 tensor;
// after it on the same stream, a fixed grid striding over the block's list
#ifndef TORJ_WARM_BIG_GRID
#define TORJ_WARM_BIG_GRID 512  // workgroups of 64: two waves per CU
#endif
template <int IWARM, bool COUNT>
__global__ void __launch_bounds__(64) k_alpha_warm_big(TraceArgs a, SplitArgs sp) {
    const unsigned cnt = *sp.defer_cnt;
    for (unsigned k = blockIdx.x * 64 + threadIdx.x; k < cnt; k += gridDim.x * 64) {
        const unsigned long long e = sp.defer[k];
        const int js = (int)(e >> 32), i = (int)(unsigned)e;
        const double *in = sp.ain + (size_t)js * kAinFW * a.n + i;
        const double Npar = in[3 * (size_t)a.n];
        const WarmSetup w = warm_setup(in[(size_t)a.n], in[2 * (size_t)a.n], Npar, in[4 * (size_t)a.n]);
        const WarmAlpha r = alpha_warm_l<IWARM, kWarmMaxL>(a.omega, in[0], in[(size_t)a.n], Npar, w,
                                                            in[5 * (size_t)a.n], a.mode);
        warm_store<COUNT>(sp, js, i, a.n, r);
    }
}

