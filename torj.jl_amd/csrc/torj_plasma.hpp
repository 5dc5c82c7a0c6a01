// torj_plasma.hpp -- the plasma handle (host): the Interpolations.jl-equivalent
// spline prefilters, torj_plasma_s, and the handle's device state created on
// first use (ensure_device, the grow-only buffers, the split pipeline's
// streams and events, the workspace budget).
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "torj_args.hpp"
#include "torj_host_util.hpp"
#include "torj_math.hpp"

// ===========================================================================
// Plasma construction (host), src/plasma.jl:16-58
// ===========================================================================
// Cubic{Line{OnGrid}} prefilter of Interpolations.jl.  The boundary rows
// c0 - 2c1 + c2 = 0 combined with the first interpolation row give c1 = y1
// (same at the far end), leaving a [1 4 1]/6 tridiagonal system for the
// interior coefficients (solved with the Thomas algorithm).
static void bspl1d_prefilter(int n, const double *y, size_t ystride, double *c, size_t cstride) {
    // c has n+2 entries
    auto C = [&](int k) -> double & { return c[(size_t)k * cstride]; };
    auto Y = [&](int k) { return y[(size_t)k * ystride]; };
    C(1) = Y(0);
    C(n) = Y(n - 1);
    const int m = n - 2;  // interior unknowns c_2..c_{n-1}
    if (m > 0) {
        std::vector<double> cp(m), dp(m);
        for (int k = 0; k < m; k++) {
            double r = 6.0 * Y(k + 1);
            if (k == 0) r -= C(1);
            if (k == m - 1) r -= C(n);
            const double den = 4.0 - (k > 0 ? cp[k - 1] : 0.0);
            cp[k] = 1.0 / den;
            dp[k] = (r - (k > 0 ? dp[k - 1] : 0.0)) / den;
        }
        C(m + 1) = dp[m - 1];
        for (int k = m - 2; k >= 0; k--) C(k + 2) = dp[k] - cp[k] * C(k + 3);
    }
    C(0) = 2.0 * C(1) - C(2);
    C(n + 1) = 2.0 * C(n) - C(n - 1);
}

// y: nR x nZ (R fastest) -> c: (nR+2) x (nZ+2) (R fastest)
static void bspl2d_prefilter(int nR, int nZ, const double *y, double *c) {
    const int mR = nR + 2, mZ = nZ + 2;
    std::fill(c, c + (size_t)mR * mZ, 0.0);
    for (int j = 0; j < nZ; j++)
        bspl1d_prefilter(nR, y + (size_t)j * nR, 1, c + (size_t)(j + 1) * mR, 1);
    std::vector<double> row(nZ);
    for (int i = 0; i < mR; i++) {
        for (int j = 0; j < nZ; j++) row[j] = c[(size_t)(j + 1) * mR + i];
        bspl1d_prefilter(nZ, row.data(), 1, c + i, (size_t)mR);
    }
}

static double bspl1d_eval(const std::vector<double> &c, int n, double x1, double xn, double x) {
    const double h = (xn - x1) / (n - 1);
    const double xc = clampd(x, x1, xn);
    const double u = (xc - x1) / h;
    int i = (int)std::floor(u);
    i = std::max(0, std::min(n - 2, i));
    double w[4], dw[4];
    bweights(u - i, w, dw);
    double v = 0, g = 0;
    for (int a = 0; a < 4; a++) {
        v += w[a] * c[i + a];
        g += dw[a] * c[i + a];
    }
    return v + (x - xc) * (g / h);
}

// natural cubic spline through (x, y) evaluated at xq (IMAS.interp1d :cubic;
// parity unpinned -- exact at the nodes, so any interpolant agrees when the
// profile grid is already uniform)
static void natcubic(int n, const double *x, const double *y, int nq, const double *xq,
                     double *yq) {
    std::vector<double> M(n, 0.0);
    if (n >= 3) {
        const int m = n - 2;
        std::vector<double> a(m), b(m), c(m), r(m);
        for (int i = 1; i <= m; i++) {
            const double h0 = x[i] - x[i - 1], h1 = x[i + 1] - x[i];
            a[i - 1] = h0;
            b[i - 1] = 2.0 * (h0 + h1);
            c[i - 1] = h1;
            r[i - 1] = 6.0 * ((y[i + 1] - y[i]) / h1 - (y[i] - y[i - 1]) / h0);
        }
        for (int i = 1; i < m; i++) {
            const double f = a[i] / b[i - 1];
            b[i] -= f * c[i - 1];
            r[i] -= f * r[i - 1];
        }
        M[m] = r[m - 1] / b[m - 1];
        for (int i = m - 1; i >= 1; i--) M[i] = (r[i - 1] - c[i - 1] * M[i + 1]) / b[i - 1];
    }
    for (int q = 0; q < nq; q++) {
        const double t = xq[q];
        const int i = std::max(0, std::min(n - 2, (int)(std::upper_bound(x, x + n, t) - x) - 1));
        if (t == x[i]) {
            yq[q] = y[i];
            continue;
        }
        if (t == x[i + 1]) {
            yq[q] = y[i + 1];
            continue;
        }
        const double h = x[i + 1] - x[i], A = x[i + 1] - t, B = t - x[i];
        yq[q] = M[i] * A * A * A / (6.0 * h) + M[i + 1] * B * B * B / (6.0 * h) +
                (y[i + 1] / h - M[i + 1] * h / 6.0) * B + (y[i] / h - M[i] * h / 6.0) * A;
    }
}

static std::vector<double> uniform_range(double a, double b, int n) {
    std::vector<double> r(n);
    for (int i = 0; i < n; i++) r[i] = a + (b - a) * i / (n - 1.0);
    r[n - 1] = b;
    return r;
}

// the 1-D half of make_2d_prof_spline (src/plasma.jl:16-22): a profile over psi resampled on
// the uniform range, taken to its logarithm and prefiltered -> c1, n_prof + 2 coefficients
static void prof1d_coefs(int n_prof, const double *psi_prof, const double *prof, std::vector<double> &c1) {
    std::vector<double> pr = uniform_range(psi_prof[0], psi_prof[n_prof - 1], n_prof);
    std::vector<double> p2(n_prof);
    c1.assign((size_t)n_prof + 2, 0.0);
    natcubic(n_prof, psi_prof, prof, n_prof, pr.data(), p2.data());
    for (double &v : p2) v = std::log(v);
    bspl1d_prefilter(n_prof, p2.data(), 1, c1.data(), 1);
}

struct torj_plasma_s {
    int device = 0;
    Grid g{};
    std::vector<double> coef;  // interleaved host copy
    // the psi_norm_data (nR x nZ, R fastest) torj_plasma_create / torj_plasma_update last
    // gave: torj_plasma_update_profiles maps new profiles through it (empty on a handle
    // whose equilibrium came as coefficients)
    std::vector<double> psi_nodes;
    double *d_coef = nullptr;
    double *d_cellp = nullptr;  // per-cell power form of coef (the cell-tiled trajectory kernel)
    int n_vol = 0;
    double v1 = 0, vn = 0;
    std::vector<double> vol_coef;
    double psi_prof_max = 0;
    hipStream_t stream = nullptr;
    GrowBuf sched;  // work-queue control block + ready-queue ring (zeroed per launch)
    int sched_mode = -1, sched_waves = 0;  // torj_set_sched
    int lanes_per_ray = 0;                 // one-shot kernel: 0 auto, 1 or 16 forced (torj_set_sched)
    GrowBuf chunk;                         // integrator 1: chunks done per ray (int)
    GrowBuf fit;                           // reference-faithful deposition workspace
    bool timing = false;                   // torj_timing: HIP events around each phase
    int timing_calls = 0;                  // trace calls recorded since torj_timing(p, 1)
    GrowBuf batch;                         // ray-batch staging of torj_trace_device_ex
    std::vector<hipEvent_t> ev_pool;       // 3 per recorded call (start, trace end, post end)
    size_t ev_used = 0;
    GrowBuf ws;                    // per-ray workspace (double: P_dep when the caller passes none)
    GrowBuf beams;                 // a multi-beam launch's beam and wave tables (BeamRec, BeamWave)
    GrowBuf mk;                    // torj_make_beams: every per-ray array of a call, launched and kept
    // sticky launch error flags, ORed by every launch since the last
    // torj_trace_check (which reads and clears them): bit 0 psi grid not
    // strictly increasing, bit 1 work-queue watchdog, bit 2 unretired groups
    int *d_flags = nullptr;
    int n_cu = 256;
    std::mutex mu;
    // torj_trace_beam: handles of the same plasma on further devices (replica k
    // on device (device + k) mod count; k = 0 is this handle) and the
    // single-process RCCL communicator over the first nccl_n of them
    std::vector<torj_plasma_s *> replicas;
    std::vector<ncclComm_t> comms;
    // torj_trace_beam's host staging on this replica (beam_worker): one or two
    // shard slots of device buffers and of host buffers (grow-only; pinned up
    // to a budget, pageable above it), the copy stream and the slots' events
    // (upload done, trace done, download done)
    struct BeamStage {
        void *d = nullptr, *h = nullptr;
        size_t d_cap = 0, h_cap = 0;
        bool h_pinned = false;
        hipStream_t sc = nullptr;
        hipEvent_t up[2] = {}, tr[2] = {}, dn[2] = {};
    } stage;
    // torj_timing of the all-reduce of make_beam's reduce (beam_reduce, host
    // clock around the grouped all-reduce and its stream waits)
    double reduce_ms = 0.0;
    int reduce_calls = 0;
    // split RK4 path: workspace, the second stream of the
    // alpha / scan kernels and the pipeline's events
    GrowBuf split;
    hipStream_t stream2 = nullptr, streamT = nullptr;  // alpha; trajectory (high priority)
    hipStream_t streamS = nullptr;                      // optical-depth scan
    hipStream_t streamD = nullptr;                      // streamed deposition windows (TORJ_DEPO_STREAM=2)
    static constexpr int kRing = kSplitRing;                  // alpha-input buffers in flight
    hipEvent_t ev_T[kRing] = {}, ev_A[kRing] = {}, ev_S[kRing] = {}, ev_J = nullptr, ev_F = nullptr;
    hipEvent_t ev_D = nullptr;
    hipEvent_t ev_Nin = nullptr, ev_Nout = nullptr;  // a NULL caller stream's fork / join
    hipEvent_t ev_U = nullptr;  // torj_plasma_update on a caller's stream: the handle's own stream waits for it
    // torj_plasma_update_gpu / _profiles_gpu / _device: the coefficients are built on
    // the device, and the host copies above go stale until a host reader asks for them (mirror_sync)
    GrowBuf cbuild;             // staging of one build: the pivots, the two 1-D profile splines, Br, Bz, Bphi
    double *d_psi = nullptr;    // the psi node map (nR x nZ), kept for profiles-only builds
    bool d_psi_valid = false;   // d_psi holds the handle's psi_nodes
    bool coef_stale = false;    // `coef` is older than d_coef
    bool psi_stale = false;     // `psi_nodes` is older than d_psi
    hipEvent_t ev_B = nullptr;  // the last build's end, which the downloads and the replicas' copies wait for
};

static const int kFieldSlot[6] = {F_PSI, F_LNNE, F_LNTE, F_BR, F_BZ, F_BPHI};

// the grid of nR x nZ nodes over the box [R1, Rn] x [Z1, Zn]
static Grid grid_box(int nR, int nZ, double R1, double Rn, double Z1, double Zn) {
    Grid g{};
    g.nR = nR;
    g.nZ = nZ;
    g.R1 = R1;
    g.Rn = Rn;
    g.Z1 = Z1;
    g.Zn = Zn;
    g.hR = (Rn - R1) / (nR - 1);
    g.hZ = (Zn - Z1) / (nZ - 1);
    g.invhR = 1.0 / g.hR;
    g.invhZ = 1.0 / g.hZ;
    return g;
}

static int plasma_finish(torj_plasma_s *p, int nR, int nZ, double R1, double Rn, double Z1,
                         double Zn, const double *const fields[6], int device,
                         torj_plasma_t *out) {
    p->device = device;
    p->g = grid_box(nR, nZ, R1, Rn, Z1, Zn);
    const size_t nodes = (size_t)(nR + 2) * (nZ + 2);
    p->coef.assign(nodes * kNF, 0.0);
    for (int f = 0; f < 6; f++)
        for (size_t k = 0; k < nodes; k++) p->coef[k * kNF + kFieldSlot[f]] = fields[f][k];
    *out = p;
    return 0;
}

// Device-side state is created on first GPU use, so the host-side parts of
// the ABI (Plasma construction, ray entry, launch fan) work without a GPU.
static int ensure_device(torj_plasma_s *p) {
    std::lock_guard<std::mutex> lk(p->mu);
    int ndev = 0;
    HIPCK(hipGetDeviceCount(&ndev));
    if (p->device < 0 || p->device >= ndev)
        return fail("device %d not available (%d HIP devices)", p->device, ndev);
    HIPCK(hipSetDevice(p->device));
    // done only once the last step below has succeeded: a handle whose earlier
    // attempt failed half-way (coefficients up, no stream) is not taken for ready
    if (p->d_flags) return 0;
    if (p->d_coef) return fail("handle's device state is incomplete (an earlier initialisation failed)");
    HIPCK(hipMalloc(&p->d_coef, p->coef.size() * sizeof(double)));
    HIPCK(hipMemcpy(p->d_coef, p->coef.data(), p->coef.size() * sizeof(double),
                    hipMemcpyHostToDevice));
    {
        std::vector<double> cp((size_t)(p->g.nR - 1) * (p->g.nZ - 1) * kCellRec);
        cell_power_table(p->coef.data(), p->g.nR, p->g.nZ, p->g.hR, p->g.hZ, cp.data());
        HIPCK(hipMalloc(&p->d_cellp, cp.size() * sizeof(double)));
        HIPCK(hipMemcpy(p->d_cellp, cp.data(), cp.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPCK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    HIPCK(hipDeviceGetAttribute(&p->n_cu, hipDeviceAttributeMultiprocessorCount, p->device));
    int *flags = nullptr;
    HIPCK(hipMalloc(&flags, sizeof(int)));
    if (hipMemset(flags, 0, sizeof(int)) != hipSuccess) {
        (void)hipFree(flags);
        return fail("hipMemset of the launch flags failed");
    }
    p->d_flags = flags;  // last: what the early return above tests
    return 0;
}

// one of the handle's grow-only buffers at `bytes` or more, under the handle's lock
static int ensure_buf(torj_plasma_s *p, GrowBuf &b, size_t bytes) {
    std::lock_guard<std::mutex> lk(p->mu);
    return b.reserve(bytes);
}

// The host copies of what a device-side build (torj_plasma_update_gpu / _profiles_gpu / _device)
// left on the device only: the host readers of `coef` and `psi_nodes` call this first.  It waits
// for the build's event and downloads, once; a later host update replaces the copies instead.
static int mirror_sync(torj_plasma_s *p) {
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->coef_stale && !p->psi_stale) return 0;
    HIPCK(hipSetDevice(p->device));
    HIPCK(hipEventSynchronize(p->ev_B));
    if (p->coef_stale) {
        HIPCK(hipMemcpy(p->coef.data(), p->d_coef, p->coef.size() * sizeof(double), hipMemcpyDeviceToHost));
        p->coef_stale = false;
    }
    if (p->psi_stale) {
        p->psi_nodes.resize((size_t)p->g.nR * p->g.nZ);
        HIPCK(hipMemcpy(p->psi_nodes.data(), p->d_psi, p->psi_nodes.size() * sizeof(double), hipMemcpyDeviceToHost));
        p->psi_stale = false;
    }
    return 0;
}

// a split-pipeline stream's priority: `dflt`, or the environment's value clamped
// to the device's range (measurement knobs: TORJ_TRAJ_PRIO, TORJ_ALPHA_PRIO,
// TORJ_SCAN_PRIO, TORJ_DEPO_PRIO; TORJ_PRIO_VERBOSE=1 prints the range)
static int stream_prio(const char *name, int dflt, int lo, int hi) {
    static const bool verbose = [&] {
        const bool on = env_int("TORJ_PRIO_VERBOSE", 0) != 0;
        if (on) fprintf(stderr, "torj: stream priority range least %d greatest %d\n", lo, hi);
        return on;
    }();
    // (dflt is lo or hi: the clamp leaves it as it is)
    const int v = std::min(std::max(env_int(name, dflt), std::min(lo, hi)), std::max(lo, hi));
    if (verbose) fprintf(stderr, "torj: %s -> %d\n", name, v);
    return v;
}

// a CU mask of k of the device's ncu CUs, spread evenly over its bits (rest: the others)
static std::vector<uint32_t> cu_mask(int ncu, int k, bool rest = false) {
    std::vector<uint32_t> m((ncu + 31) / 32, 0u);
    for (int c = 0; c < ncu; c++)
        if ((((long)(c + 1) * k) / ncu != ((long)c * k) / ncu) != rest) m[c / 32] |= 1u << (c % 32);
    return m;
}

static int ensure_split(torj_plasma_s *p, size_t bytes) {
    std::lock_guard<std::mutex> lk(p->mu);
    if (!p->stream2) {
        // the trajectory chain is the critical path: its stream gets the highest
        // priority, so its waves are dispatched ahead of the alpha kernel's
        int lo = 0, hi = 0;
        HIPCK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        // TORJ_TRAJ_CUS=X: the trajectory stream on X of the device's CUs (evenly
        // spread over the mask's bits), the alpha and scan streams on the rest
        int dev = 0, ncu = 0;
        HIPCK(hipGetDevice(&dev));
        HIPCK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
        const int X = env_int("TORJ_TRAJ_CUS", 0), Y = env_int("TORJ_ALPHA_CUS", 0);
        if (Y > 0 && Y < ncu) {
            // TORJ_ALPHA_CUS=Y: only the alpha and scan streams masked (to Y CUs),
            // the trajectory stream on every CU -- the others never hold alpha waves
            const std::vector<uint32_t> mA = cu_mask(ncu, Y);
            HIPCK(hipStreamCreateWithPriority(&p->streamT, hipStreamNonBlocking, hi));
            HIPCK(hipExtStreamCreateWithCUMask(&p->stream2, (uint32_t)mA.size(), mA.data()));
            HIPCK(hipExtStreamCreateWithCUMask(&p->streamS, (uint32_t)mA.size(), mA.data()));
        } else if (X > 0 && X < ncu) {
            const std::vector<uint32_t> mT = cu_mask(ncu, X), mA = cu_mask(ncu, X, true);
            HIPCK(hipExtStreamCreateWithCUMask(&p->streamT, (uint32_t)mT.size(), mT.data()));
            HIPCK(hipExtStreamCreateWithCUMask(&p->stream2, (uint32_t)mA.size(), mA.data()));
            HIPCK(hipExtStreamCreateWithCUMask(&p->streamS, (uint32_t)mA.size(), mA.data()));
        } else {
            HIPCK(hipStreamCreateWithPriority(&p->streamT, hipStreamNonBlocking, stream_prio("TORJ_TRAJ_PRIO", hi, lo, hi)));
            HIPCK(hipStreamCreateWithPriority(&p->stream2, hipStreamNonBlocking, stream_prio("TORJ_ALPHA_PRIO", lo, lo, hi)));
            // TORJ_SCAN_CUS=Z (measurement knob): the scan's stream -- the optical-depth
            // scan and the streamed deposition's elimination and walk, latency-bound
            // waves of up to 168 VGPRs -- on Z evenly spread CUs only, so the others
            // keep their registers for the alpha waves
            const int Z = env_int("TORJ_SCAN_CUS", 0);
            if (Z > 0 && Z < ncu) {
                const std::vector<uint32_t> mS = cu_mask(ncu, Z);
                HIPCK(hipExtStreamCreateWithCUMask(&p->streamS, (uint32_t)mS.size(), mS.data()));
            } else {
                HIPCK(hipStreamCreateWithPriority(&p->streamS, hipStreamNonBlocking, stream_prio("TORJ_SCAN_PRIO", lo, lo, hi)));
            }
        }
        for (int q = 0; q < torj_plasma_s::kRing; q++) {
            HIPCK(hipEventCreateWithFlags(&p->ev_T[q], hipEventDisableTiming));
            HIPCK(hipEventCreateWithFlags(&p->ev_A[q], hipEventDisableTiming));
            HIPCK(hipEventCreateWithFlags(&p->ev_S[q], hipEventDisableTiming));
        }
        HIPCK(hipEventCreateWithFlags(&p->ev_J, hipEventDisableTiming));
        HIPCK(hipEventCreateWithFlags(&p->ev_F, hipEventDisableTiming));
        HIPCK(hipEventCreateWithFlags(&p->ev_D, hipEventDisableTiming));
    }
    return p->split.reserve(bytes);
}

// Device-memory budget of one launch's per-ray workspace (the reference
// deposition's per-step samples and elimination coefficients, root counts and
// shell arrays: ~116 KB per ray at 2 000 steps and 1 000 shells).  A beam whose
// workspace would exceed it is traced in contiguous batches of whole 64-ray
// groups, each batch's inputs gathered into and outputs scattered from
// compact device buffers.  TORJ_WS_GB (read per call, tests vary it) sets the
// budget; by default it is half of the device memory this handle could use
// (free + its own fit workspace, which a larger one replaces), at least 16 GiB:
// on a 288 GB MI355X the 1e6-ray C4 beam (~116 GB) then runs as one launch
// (606 against 675 ms in seven 16 GiB batches, each with its own pipeline fill
// and drain), with room left for the split ring and the caller's buffers.
// The device must be current (ensure_device).
static size_t ws_budget(const torj_plasma_s *p) {
    if (env_has("TORJ_WS_GB")) return (size_t)(env_double("TORJ_WS_GB", 0.0) * (double)(1ull << 30));
    const size_t floor16 = 16ull << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return floor16;
    return std::max(floor16, (free_b + p->fit.cap) / 2);
}

