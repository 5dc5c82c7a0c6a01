// torj_hip.hip -- libtorj_hip.so's main translation unit: the C ABI declared in
// include/torj_hip.h.  The kernels and the host layers are headers, cut along
// the include graph:
//   torj_args.hpp       TraceArgs / SplitArgs and the compile-time launch shapes
//   torj_k_fused.hpp    k_trace, the Tsit5 queue kernel k_trace_sched, c_gl
//   torj_k_traj.hpp     the split pipeline's trajectory kernels
//   torj_k_alpha.hpp    ... its alpha kernels
//   torj_k_scan.hpp     ... its optical-depth scan and final assembly
//   torj_k_depo.hpp     the reference-faithful deposition's kernels
//   torj_k_points.hpp   ray entry and the batched point evaluations
//   torj_k_beams.hpp    the multi-beam forms of k_trace and the kernels around it,
//                       also for beams that go through differing plasmas
//   torj_celltab.hpp    the cell table rebuilt on the device (torj_plasma_update*)
//   torj_coefbuild.hpp  the node coefficients built on the device (torj_plasma_update_gpu,
//                       _profiles_gpu, _device): one prefilter line, one profile node, their kernels
//   torj_host_util.hpp  fail / HIPCK, the environment knobs, GrowBuf
//   torj_plasma.hpp     the plasma handle and its device state
//   torj_fan.hpp        quadrature nodes and the launch fan
//   torj_dispatch.hpp   run-time (absorption, deposition, trajectory) -> kernel instance
//   torj_split.hpp      the split pipeline's launches (split_trace)
//   torj_launch.hpp     one launch of the hot path: LaunchPlan, FitLayout, RayIO,
//                       trace_device (one launch or ray batches), the Gauss-Legendre upload
//   torj_beam.hpp       torj_trace_beam's multi-device layer
// Here: the Gauss-Legendre table's construction and the extern "C" functions, which name a
// call's arrays into a RayIO (ray entry: EntryIO) once; every host layer below takes the struct.
// k_traj_cell is compiled in torj_traj.hip with flags of its own (-DTORJ_TRAJ_OWN_TU=1
// here, csrc/Makefile); without that define this file is the whole library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/torj_hip.h"
#include "torj_math.hpp"
#include "torj_entry.hpp"
#include "torj_fitdepo.hpp"
#include "torj_warm.hpp"

using namespace torj;

#include "torj_host_util.hpp"
#include "torj_args.hpp"
#include "torj_k_fused.hpp"
#include "torj_k_traj.hpp"
#include "torj_k_alpha.hpp"
#include "torj_k_scan.hpp"
#include "torj_k_depo.hpp"
#include "torj_k_points.hpp"
#include "torj_k_beams.hpp"
#include "torj_celltab.hpp"
#include "torj_coefbuild.hpp"
#include "torj_plasma.hpp"
#include "torj_fan.hpp"
#include "torj_split.hpp"
#include "torj_launch.hpp"
#include "torj_beam.hpp"

// ===========================================================================
// host-pointer entries: the arrays staged around a device-pointer call
// ===========================================================================
// a host copy of psi_dP_dV, checked before any device work (the device copies: k_grid_check)
static int grid_increasing(int n_psi, const double *grid) {
    for (int k = 1; k < n_psi; k++)
        if (!(grid[k] > grid[k - 1])) return fail("psi_dP_dV must be strictly increasing");
    return 0;
}

// A trace of the h.n > 0 rays in the host arrays h with n_dP rows of dP_shell: uploads,
// allocations, the zeroed dP, `call(d, n_psi, s)` -- the device-pointer trace on h's device
// copies d, n_psi 0 without deposition -- then the downloads (zeros where there was no
// deposition) and torj_trace_check.  Synchronous.
template <class F>
static int trace_staged(torj_plasma_t p, const torj_trace_cfg *cfg, const RayIO &h, int n_dP, int n_psi, F call) {
    const int n = h.n;
    const bool depo = n_psi >= 2 && h.psi_grid;
    const size_t rows = dP_rows(n_dP, n_psi);
    if (ensure_device(p)) return -1;
    hipStream_t s = p->stream;
    const int n_save = cfg->traj_stride > 0 ? cfg->n_steps / cfg->traj_stride : 0;
    DevBufs B;
    RayIO d{n};  // each array's device copy under its own name; no counters
    if (B.up(&d.x0, h.x0, 3 * (size_t)n, s) || B.up(&d.N0, h.N0, 3 * (size_t)n, s) ||
        B.up(&d.weights, h.weights, n, s) || B.up(&d.x_launch, h.x_launch, 3 * (size_t)n, s) || B.up(&d.s0, h.s0, n, s))
        return -1;
    if (depo) {
        if (B.up(&d.psi_grid, h.psi_grid, n_psi, s) || B.alloc(&d.dP_shell, rows, true) || B.alloc(&d.P_dep, n, true))
            return -1;
        HIPCK(hipMemsetAsync(d.dP_shell, 0, rows * sizeof(double), s));
    }
    if (B.alloc(&d.state, 7 * (size_t)n, true) || B.alloc(&d.status, n, true) || B.alloc(&d.steps, n, true) ||
        B.alloc(&d.traj, (size_t)n_save * 5 * n, h.traj && n_save > 0))
        return -1;
    if (call(d, depo ? n_psi : 0, s)) return -1;
    if (ddownload(h.state, d.state, 7 * (size_t)n, s) || ddownload(h.status, d.status, n, s) ||
        ddownload(h.steps, d.steps, n, s))
        return -1;
    if (depo) {
        if (ddownload(h.dP_shell, d.dP_shell, rows, s) || ddownload(h.P_dep, d.P_dep, n, s)) return -1;
    } else {
        if (h.dP_shell) std::fill(h.dP_shell, h.dP_shell + rows, 0.0);
        if (h.P_dep) std::fill(h.P_dep, h.P_dep + n, 0.0);
    }
    if (h.traj && n_save > 0 && ddownload(h.traj, d.traj, (size_t)n_save * 5 * n, s)) return -1;
    return torj_trace_check(p, s);
}

struct EntryIO {  // the ray entry's arrays, as torj_ray_entry_device takes them
    int n;
    const double *x0, *N0;
    double *xp, *Np, *s0;
    int *status;
};

// The ray entry of the h.n > 0 rays of the host arrays h: `call(d, s)` is the device-pointer
// entry on their device copies d.  Synchronous.
template <class F>
static int entry_staged(torj_plasma_t p, const EntryIO &h, F call) {
    if (ensure_device(p)) return -1;
    hipStream_t s = p->stream;
    const size_t n = (size_t)h.n;
    DevBufs B;
    EntryIO d{h.n};
    if (B.up(&d.x0, h.x0, 3 * n, s) || B.up(&d.N0, h.N0, 3 * n, s)) return -1;
    if (B.alloc(&d.xp, 3 * n, true) || B.alloc(&d.Np, 3 * n, true) || B.alloc(&d.s0, n, true) ||
        B.alloc(&d.status, n, true))
        return -1;
    if (call(d, s)) return -1;
    if (ddownload(h.xp, d.xp, 3 * n, s) || ddownload(h.Np, d.Np, 3 * n, s) || ddownload(h.s0, d.s0, n, s) ||
        ddownload(h.status, d.status, n, s))
        return -1;
    HIPCK(hipStreamSynchronize(s));
    return 0;
}

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int torj_abi_version(void) { return TORJ_ABI_VERSION; }

#ifndef TORJ_BUILD_ID
#define TORJ_BUILD_ID "unstamped"
#endif
const char *torj_build_id(void) { return TORJ_BUILD_ID; }

#ifdef TORJ_ALPHA_PROF
// profiling build only (not in include/torj_hip.h): g_aprof, read and reset
int torj_alpha_prof_read(unsigned long long *out) {
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_aprof), sizeof(g_aprof)));
    static const unsigned long long zero[16] = {};
    HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_aprof), zero, sizeof(g_aprof)));
    return 0;
}
#endif
#ifdef TORJ_WARM_PROF
// profiling build only (not in include/torj_hip.h): the warm alpha's region
// timers -- out[0] waves, out[1 + k] clock ticks of region k -- read and reset
int torj_warm_prof_read(unsigned long long *out) {
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wprof), sizeof(g_wprof)));
    static const unsigned long long zero[kWProfN + 1] = {};
    HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_wprof), zero, sizeof(g_wprof)));
    return 0;
}
int torj_warm_fad_read(unsigned long long *out) {
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wfad), sizeof(g_wfad)));
    static const unsigned long long zero[9] = {};
    HIPCK(hipMemcpyToSymbol(HIP_SYMBOL(g_wfad), zero, sizeof(g_wfad)));
    return 0;
}
#endif

const char *torj_last_error(void) { return g_err.c_str(); }

int torj_device_count(int *n) {
    HIPCK(hipGetDeviceCount(n));
    return 0;
}

int torj_abs_al_init(int n) {
    if (n < 1 || n > kMaxGL) return fail("abs_Al_init: order %d outside [1, %d]", n, kMaxGL);
    std::lock_guard<std::mutex> lk(g_gl_mu);
    GLTable t{};
    t.n = n;
    // the bit-identical skip of provably negligible harmonic integrals
    // (torj_math.hpp albajar_harmonic); env TORJ_NEGL_SKIP=0 turns it off (A/B
    // and the test that holds both bit-identical), read at each abs_Al_init
    t.negl_skip = env_int("TORJ_NEGL_SKIP", 1) != 0;
    // harmonic 3 dismissed from the prologue's outputs where its skip is certain
    // (torj_math.hpp h3_fast_negligible; bit-identical, uncounted launches);
    // env TORJ_H3_FAST=0 turns it off, and so does TORJ_NEGL_SKIP=0
    t.h3_fast = t.negl_skip && env_int("TORJ_H3_FAST", 1) != 0;
    // the bounded skip of a harmonic whose share of alpha is provably below
    // tiny_alpha m^-1 (albajar_harmonic; ray tracing only -- the point entry
    // torj_abs_albajar_fast evaluates every harmonic): tau moves by less than
    // 2 tiny_alpha per metre of ray, 4e-21 on the headline rays, against the
    // parity bar's 1e-16 absolute floor (C3 trace phase 45.1 -> 40.7 ms, DESIGN.md
    // 3.7).  Env TORJ_TINY_ALPHA overrides (0 = off: every integral evaluated),
    // read at each abs_Al_init
    t.tiny_alpha = env_double("TORJ_TINY_ALPHA", kTinyAlpha);
    if (!(t.tiny_alpha >= 0.0 && t.tiny_alpha < 1e-12)) return fail("TORJ_TINY_ALPHA=%g outside [0, 1e-12)", t.tiny_alpha);
    gauss_legendre(n, t.t, t.w);
    for (int i = 0; i < n; i++) {
        t.st[i] = std::sqrt(1.0 - t.t[i] * t.t[i]);
        t.t2[i] = t.t[i] * t.t[i];
        gl_node_consts(t, i);
    }
    g_gl_host = t;
    g_gl_version++;
    return 0;
}

}  // extern "C"

// make_2d_prof_spline (src/plasma.jl:16-22): a 1-D profile over psi, resampled on the uniform
// range and taken to its logarithm, mapped through the nodes' psi_norm -> 2-D coefficients
static void prof2d_coefs(int nR, int nZ, const double *psi_norm, int n_prof, const double *psi_prof,
                         const double *prof, std::vector<double> &c2) {
    const size_t nd = (size_t)nR * nZ;
    std::vector<double> c1, d2(nd);
    prof1d_coefs(n_prof, psi_prof, prof, c1);
    for (size_t k = 0; k < nd; k++)
        d2[k] = bspl1d_eval(c1, n_prof, psi_prof[0], psi_prof[n_prof - 1], psi_norm[k]);
    bspl2d_prefilter(nR, nZ, d2.data(), c2.data());
}

// The host state of a plasma from its node data, into the blank handle p: the body of
// torj_plasma_create, and of torj_plasma_update on a scratch handle (plasma_adopt)
static int plasma_from_maps(torj_plasma_s *p, int nR, int nZ, const double *R, const double *Z,
                            const double *psi_norm, int n_prof, const double *psi_prof, const double *ne_prof,
                            const double *Te_prof, const double *Br, const double *Bz, const double *Bphi,
                            int n_eq, const double *eq_psi, const double *eq_vol, int device) {
    const size_t nc = (size_t)(nR + 2) * (nZ + 2);
    std::vector<double> cpsi(nc), cne(nc), cte(nc), cbr(nc), cbz(nc), cbp(nc);
    bspl2d_prefilter(nR, nZ, psi_norm, cpsi.data());
    bspl2d_prefilter(nR, nZ, Br, cbr.data());
    bspl2d_prefilter(nR, nZ, Bz, cbz.data());
    bspl2d_prefilter(nR, nZ, Bphi, cbp.data());
    prof2d_coefs(nR, nZ, psi_norm, n_prof, psi_prof, ne_prof, cne);
    prof2d_coefs(nR, nZ, psi_norm, n_prof, psi_prof, Te_prof, cte);
    // volume_psi_spline (src/plasma.jl:42-44)
    std::vector<double> pr = uniform_range(eq_psi[0], eq_psi[n_eq - 1], n_eq), v2(n_eq);
    natcubic(n_eq, eq_psi, eq_vol, n_eq, pr.data(), v2.data());
    p->n_vol = n_eq;
    p->v1 = eq_psi[0];
    p->vn = eq_psi[n_eq - 1];
    p->vol_coef.assign(n_eq + 2, 0.0);
    bspl1d_prefilter(n_eq, v2.data(), 1, p->vol_coef.data(), 1);
    p->psi_prof_max = *std::max_element(psi_prof, psi_prof + n_prof);
    p->psi_nodes.assign(psi_norm, psi_norm + (size_t)nR * nZ);
    const double *fields[6] = {cpsi.data(), cne.data(), cte.data(), cbr.data(), cbz.data(), cbp.data()};
    torj_plasma_t out;
    return plasma_finish(p, nR, nZ, R[0], R[nR - 1], Z[0], Z[nZ - 1], fields, device, &out);
}

// ... and from Interpolations.jl coefficients (torj_plasma_create_from_coefs, torj_plasma_update_from_coefs)
static int plasma_from_coefs(torj_plasma_s *p, int nR, int nZ, double R1, double Rn, double Z1, double Zn,
                             const double *c_psi, const double *c_lnne, const double *c_lnTe, const double *c_Br,
                             const double *c_Bz, const double *c_Bphi, int n_vol, double vol_psi1,
                             double vol_psin, const double *vol_coefs, double psi_prof_max, int device) {
    p->n_vol = n_vol;
    p->v1 = vol_psi1;
    p->vn = vol_psin;
    p->vol_coef.assign(vol_coefs, vol_coefs + n_vol + 2);
    p->psi_prof_max = psi_prof_max;
    const double *fields[6] = {c_psi, c_lnne, c_lnTe, c_Br, c_Bz, c_Bphi};
    torj_plasma_t out;
    return plasma_finish(p, nR, nZ, R1, Rn, Z1, Zn, fields, device, &out);
}

// ===========================================================================
// torj_plasma_update*: a live handle's physics replaced
// ===========================================================================
// the device half, on one handle or replica whose device state exists: the new
// coefficients into d_coef (from pageable memory, consumed when the copy returns:
// beams_upload's rule), then d_cellp rebuilt from them, both in `s`'s order
static int cell_table_enqueue(torj_plasma_s *q, hipStream_t s);
static int plasma_update_enqueue(torj_plasma_s *q, hipStream_t s) {
    HIPCK(hipMemcpyAsync(q->d_coef, q->coef.data(), q->coef.size() * sizeof(double), hipMemcpyHostToDevice, s));
    return cell_table_enqueue(q, s);
}
// d_cellp rebuilt from d_coef in `s`'s order
static int cell_table_enqueue(torj_plasma_s *q, hipStream_t s) {
    const long n = (long)(q->g.nR - 1) * (q->g.nZ - 1) * kCellNS;
    hipLaunchKernelGGL(k_cell_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q->d_coef, q->g, q->d_cellp);
    HIPCK(hipGetLastError());
    return 0;
}

// The complete new host state in `fresh` (a scratch handle, the same grid size) becomes p's and
// its replicas'; where device state exists the device half follows: the handle's on the caller's
// stream (NULL: on_caller_stream's fork and join), each replica's on its own device and stream.
// Nothing waits for the device.
static int plasma_adopt(torj_plasma_s *p, torj_plasma_s &fresh, void *stream) {
    std::vector<torj_plasma_s *> live;  // handles whose device state exists
    {
        std::lock_guard<std::mutex> lk(p->mu);
        for (size_t k = 0; k < std::max<size_t>(1, p->replicas.size()); k++) {
            torj_plasma_s *q = k == 0 ? p : p->replicas[k];
            q->g = fresh.g;
            q->coef = fresh.coef;
            q->n_vol = fresh.n_vol, q->v1 = fresh.v1, q->vn = fresh.vn;
            q->vol_coef = fresh.vol_coef;
            q->psi_prof_max = fresh.psi_prof_max;
            q->coef_stale = false;  // (a device-side build's mirror: replaced, not downloaded)
            if (q->d_flags) live.push_back(q);
        }
        p->psi_nodes.swap(fresh.psi_nodes);
        p->psi_stale = false;
        p->d_psi_valid = false;
    }
    int rc = 0;
    for (torj_plasma_s *q : live) {
        if (hipSetDevice(q->device) != hipSuccess) {
            rc = fail("hipSetDevice(%d) failed", q->device);
            break;
        }
        if (q != p) {
            rc = plasma_update_enqueue(q, q->stream);
        } else {
            rc = on_caller_stream(p, stream, [&](hipStream_t s) {
                if (plasma_update_enqueue(p, s)) return -1;
                if (s == p->stream) return 0;
                // the host-pointer entries run on the handle's own stream: it waits for this update
                if (!p->ev_U) HIPCK(hipEventCreateWithFlags(&p->ev_U, hipEventDisableTiming));
                HIPCK(hipEventRecord(p->ev_U, s));
                HIPCK(hipStreamWaitEvent(p->stream, p->ev_U, 0));
                return 0;
            });
        }
        if (rc) break;
    }
    if (live.size() > 1 || (live.size() == 1 && live[0] != p)) (void)hipSetDevice(p->device);
    return rc;
}

// ===========================================================================
// torj_plasma_update_gpu, _profiles_gpu, _device: the 2-D coefficients built on
// the device (torj_coefbuild.hpp)
// ===========================================================================
// (cb_field_slot's nibbles against kFieldSlot itself: tests/native/coefbuild_host.hip cb_slots_ok)
static_assert(F_PSI == 5 && F_LNNE == 3 && F_LNTE == 4 && F_BR == 0 && F_BZ == 2 && F_BPHI == 1,
              "cb_field_slot's nibbles are kFieldSlot's values");

// The 1-D host state of an update, complete before the handle is touched: the two ln-profile
// splines (today's host functions: glibc's log and the device's differ in the last bit),
// psi_prof_max, and for a full update the box and the volume spline.
struct Update1D {
    bool full = false;
    int n_prof = 0;
    double x1 = 0, xn = 0, psi_prof_max = 0;
    std::vector<double> c1_ne, c1_te;
    Grid g{};
    int n_vol = 0;
    double v1 = 0, vn = 0;
    std::vector<double> vol_coef;
};
static void update1d_profiles(Update1D &u, int n_prof, const double *psi_prof, const double *ne_prof,
                              const double *Te_prof) {
    u.n_prof = n_prof;
    u.x1 = psi_prof[0], u.xn = psi_prof[n_prof - 1];
    prof1d_coefs(n_prof, psi_prof, ne_prof, u.c1_ne);
    prof1d_coefs(n_prof, psi_prof, Te_prof, u.c1_te);
    u.psi_prof_max = *std::max_element(psi_prof, psi_prof + n_prof);
}
static void update1d_full(Update1D &u, int nR, int nZ, const double *R, const double *Z, int n_eq,
                          const double *eq_psi, const double *eq_vol) {
    u.full = true;
    u.g = grid_box(nR, nZ, R[0], R[nR - 1], Z[0], Z[nZ - 1]);
    // volume_psi_spline (src/plasma.jl:42-44), as plasma_from_maps
    std::vector<double> pr = uniform_range(eq_psi[0], eq_psi[n_eq - 1], n_eq), v2(n_eq);
    natcubic(n_eq, eq_psi, eq_vol, n_eq, pr.data(), v2.data());
    u.n_vol = n_eq;
    u.v1 = eq_psi[0];
    u.vn = eq_psi[n_eq - 1];
    u.vol_coef.assign(n_eq + 2, 0.0);
    bspl1d_prefilter(n_eq, v2.data(), 1, u.vol_coef.data(), 1);
}

// where a build's node maps are: host arrays (psi, Br, Bz, Bphi; consumed before the call returns),
// device arrays read in stream order, or neither (profiles only: the handle's own psi nodes)
struct BuildMaps {
    const double *host[4] = {nullptr, nullptr, nullptr, nullptr};
    const double *dev[4] = {nullptr, nullptr, nullptr, nullptr};
};

// The build on `s`: staging copies, the three kernels into d_coef, k_cell_table; ev_B at its end.
// Then each live replica's device copy of d_coef (a peer copy across devices) and its own
// k_cell_table on its own stream, behind ev_B; `s` waits for those copies, so that a later
// build on it cannot overwrite d_coef under them.
static int plasma_build_enqueue(torj_plasma_s *p, const Update1D &u, const BuildMaps &m, hipStream_t s,
                                const std::vector<torj_plasma_s *> &live) {
    const int nR = p->g.nR, nZ = p->g.nZ;
    const size_t nd = (size_t)nR * nZ, ncp = (size_t)std::max(nR, nZ), n1 = (size_t)u.n_prof + 2;
    double *stg = (double *)p->cbuild.d;
    // the small block: pivots and the two 1-D splines, packed into one copy from pageable memory
    std::vector<double> small(ncp + 2 * n1, 0.0);
    cb_pivots(std::max(nR, nZ) - 2, small.data());
    std::copy(u.c1_ne.begin(), u.c1_ne.end(), small.begin() + ncp);
    std::copy(u.c1_te.begin(), u.c1_te.end(), small.begin() + ncp + n1);
    HIPCK(hipMemcpyAsync(stg, small.data(), small.size() * sizeof(double), hipMemcpyHostToDevice, s));
    CoefBuild a{};
    a.coef = p->d_coef;
    a.cp = stg, a.c1_ne = stg + ncp, a.c1_te = stg + ncp + n1;
    a.psi = p->d_psi;
    a.x1 = u.x1, a.xn = u.xn, a.n_prof = u.n_prof, a.nR = nR, a.nZ = nZ;
    a.f0 = u.full ? 0 : 1, a.nf = u.full ? 6 : 2;
    if (m.host[0]) {
        double *maps = stg + small.size();
        HIPCK(hipMemcpyAsync(p->d_psi, m.host[0], nd * sizeof(double), hipMemcpyHostToDevice, s));
        for (int k = 1; k < 4; k++)
            HIPCK(hipMemcpyAsync(maps + (size_t)(k - 1) * nd, m.host[k], nd * sizeof(double), hipMemcpyHostToDevice, s));
        a.Br = maps, a.Bz = maps + nd, a.Bphi = maps + 2 * nd;
    } else if (m.dev[0]) {
        HIPCK(hipMemcpyAsync(p->d_psi, m.dev[0], nd * sizeof(double), hipMemcpyDeviceToDevice, s));
        a.Br = m.dev[1], a.Bz = m.dev[2], a.Bphi = m.dev[3];
    } else if (!p->d_psi_valid) {  // profiles only, first need: the host copy of the psi nodes
        HIPCK(hipMemcpyAsync(p->d_psi, p->psi_nodes.data(), nd * sizeof(double), hipMemcpyHostToDevice, s));
    }
    p->d_psi_valid = true;
    const long n_nodes = (long)nd * a.nf;
    hipLaunchKernelGGL(k_coef_nodes, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_coef_prefilter, dim3((unsigned)nblocks(nZ * a.nf, 64)), dim3(64), 0, s, a, false);
    hipLaunchKernelGGL(k_coef_prefilter, dim3((unsigned)nblocks((nR + 2) * a.nf, 64)), dim3(64), 0, s, a, true);
    HIPCK(hipGetLastError());
    if (cell_table_enqueue(p, s)) return -1;
    if (!p->ev_B) HIPCK(hipEventCreateWithFlags(&p->ev_B, hipEventDisableTiming));
    HIPCK(hipEventRecord(p->ev_B, s));
    // the host-pointer entries run on the handle's own stream: it waits for this build
    if (s != p->stream) HIPCK(hipStreamWaitEvent(p->stream, p->ev_B, 0));
    for (torj_plasma_s *q : live) {
        if (q == p) continue;
        const size_t bytes = p->coef.size() * sizeof(double);
        HIPCK(hipSetDevice(q->device));
        HIPCK(hipStreamWaitEvent(q->stream, p->ev_B, 0));
        if (q->device == p->device)
            HIPCK(hipMemcpyAsync(q->d_coef, p->d_coef, bytes, hipMemcpyDeviceToDevice, q->stream));
        else
            HIPCK(hipMemcpyPeerAsync(q->d_coef, q->device, p->d_coef, p->device, bytes, q->stream));
        if (cell_table_enqueue(q, q->stream)) return -1;
        if (!q->ev_U) HIPCK(hipEventCreateWithFlags(&q->ev_U, hipEventDisableTiming));
        HIPCK(hipEventRecord(q->ev_U, q->stream));
        HIPCK(hipSetDevice(p->device));
        HIPCK(hipStreamWaitEvent(s, q->ev_U, 0));
    }
    return 0;
}

// The device-side counterpart of plasma_adopt.  `who` names the entry in messages.  The handle gets
// its device state if it has none; the staging buffers are sized; then the 1-D state becomes the
// handle's and its replicas', their host coefficients (and, for device maps, the psi nodes) are
// marked stale, and the build is enqueued on the caller's stream.  Nothing waits for the device.
static int plasma_build(torj_plasma_s *p, const char *who, const Update1D &u, const BuildMaps &m, void *stream) {
    const size_t nd = (size_t)p->g.nR * p->g.nZ;
    std::vector<torj_plasma_s *> live;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        const size_t need = (size_t)std::max(p->g.nR, p->g.nZ) + 2 * ((size_t)u.n_prof + 2) + (m.host[0] ? 3 * nd : 0);
        if (p->cbuild.reserve(need * sizeof(double))) return -1;
        if (!p->d_psi) HIPCK(hipMalloc(&p->d_psi, nd * sizeof(double)));
        for (size_t k = 0; k < std::max<size_t>(1, p->replicas.size()); k++) {
            torj_plasma_s *q = k == 0 ? p : p->replicas[k];
            if (u.full) {
                q->g = u.g;
                q->n_vol = u.n_vol, q->v1 = u.v1, q->vn = u.vn;
                q->vol_coef = u.vol_coef;
            }
            q->psi_prof_max = u.psi_prof_max;
            q->coef_stale = true;
            if (q->d_flags) live.push_back(q);
        }
        if (m.host[0]) {
            p->psi_nodes.assign(m.host[0], m.host[0] + nd);
            p->psi_stale = false;
        } else if (m.dev[0]) {
            p->psi_stale = true;
        }
    }
    const int rc = on_caller_stream(p, stream, [&](hipStream_t s) { return plasma_build_enqueue(p, u, m, s, live); });
    if (live.size() > 1) (void)hipSetDevice(p->device);
    if (rc) return fail("%s: %s", who, std::string(g_err).c_str());
    return 0;
}

// the checks the three entries share, before anything else: the arguments by name (build_checks), then a
// usable GPU (build_device: the handle's device state, created here on its first GPU use)
struct NamedPtr {
    const char *name;
    const void *ptr;
};
static int build_checks(torj_plasma_s *p, const char *who, const NamedPtr *args, size_t n_args, int n_prof,
                        const int *n_eq) {
    if (!p) return fail("%s: p is NULL", who);
    for (size_t k = 0; k < n_args; k++)
        if (!args[k].ptr) return fail("%s: %s is NULL", who, args[k].name);
    if (n_prof < 2) return fail("%s: n_prof = %d < 2", who, n_prof);
    if (n_eq && *n_eq < 2) return fail("%s: n_eq = %d < 2", who, *n_eq);
    return 0;
}
static int build_device(torj_plasma_s *p, const char *who) {
    if (ensure_device(p)) return fail("%s: no usable GPU for the handle (%s)", who, std::string(g_err).c_str());
    return 0;
}

extern "C" {

int torj_plasma_create(int nR, int nZ, const double *R, const double *Z, const double *psi_norm,
                       int n_prof, const double *psi_prof, const double *ne_prof,
                       const double *Te_prof, const double *Br, const double *Bz,
                       const double *Bphi, int n_eq, const double *eq_psi, const double *eq_vol,
                       int device, torj_plasma_t *out) {
    if (!out) return fail("out is NULL");
    if (nR < 2 || nZ < 2 || n_prof < 2 || n_eq < 2) return fail("Plasma: grids need >= 2 points");
    auto *p = new torj_plasma_s();
    const int rc = plasma_from_maps(p, nR, nZ, R, Z, psi_norm, n_prof, psi_prof, ne_prof, Te_prof, Br, Bz, Bphi,
                                    n_eq, eq_psi, eq_vol, device);
    if (rc)
        delete p;
    else
        *out = p;
    return rc;
}

int torj_plasma_create_from_coefs(int nR, int nZ, double R1, double Rn, double Z1, double Zn,
                                  const double *c_psi, const double *c_lnne, const double *c_lnTe,
                                  const double *c_Br, const double *c_Bz, const double *c_Bphi,
                                  int n_vol, double vol_psi1, double vol_psin,
                                  const double *vol_coefs, double psi_prof_max, int device,
                                  torj_plasma_t *out) {
    if (!out) return fail("out is NULL");
    if (nR < 2 || nZ < 2 || n_vol < 2) return fail("Plasma: grids need >= 2 points");
    auto *p = new torj_plasma_s();
    const int rc = plasma_from_coefs(p, nR, nZ, R1, Rn, Z1, Zn, c_psi, c_lnne, c_lnTe, c_Br, c_Bz, c_Bphi, n_vol,
                                     vol_psi1, vol_psin, vol_coefs, psi_prof_max, device);
    if (rc)
        delete p;
    else
        *out = p;
    return rc;
}

// every refusal before the handle is touched; the new state whole in a scratch handle, then adopted
int torj_plasma_update(torj_plasma_t p, const double *R, const double *Z, const double *psi_norm, int n_prof,
                       const double *psi_prof, const double *ne_prof, const double *Te_prof, const double *Br,
                       const double *Bz, const double *Bphi, int n_eq, const double *eq_psi,
                       const double *eq_vol, void *stream) {
    if (!p) return fail("torj_plasma_update: p is NULL");
    const struct {
        const char *name;
        const void *ptr;
    } args[] = {{"R_coords", R},     {"Z_coords", Z},   {"psi_norm_data", psi_norm}, {"psi_prof", psi_prof},
                {"ne_prof", ne_prof}, {"Te_prof", Te_prof}, {"Br_data", Br},          {"Bz_data", Bz},
                {"Bphi_data", Bphi}, {"eqt1d_psi_norm", eq_psi}, {"eqt1d_volume", eq_vol}};
    for (const auto &a : args)
        if (!a.ptr) return fail("torj_plasma_update: %s is NULL", a.name);
    if (n_prof < 2) return fail("torj_plasma_update: n_prof = %d < 2", n_prof);
    if (n_eq < 2) return fail("torj_plasma_update: n_eq = %d < 2", n_eq);
    torj_plasma_s fresh;
    if (plasma_from_maps(&fresh, p->g.nR, p->g.nZ, R, Z, psi_norm, n_prof, psi_prof, ne_prof, Te_prof, Br, Bz, Bphi,
                         n_eq, eq_psi, eq_vol, p->device))
        return -1;
    return plasma_adopt(p, fresh, stream);
}

int torj_plasma_update_from_coefs(torj_plasma_t p, double R1, double Rn, double Z1, double Zn,
                                  const double *c_psi, const double *c_lnne, const double *c_lnTe,
                                  const double *c_Br, const double *c_Bz, const double *c_Bphi, int n_vol,
                                  double vol_psi1, double vol_psin, const double *vol_coefs, double psi_prof_max,
                                  void *stream) {
    if (!p) return fail("torj_plasma_update_from_coefs: p is NULL");
    const struct {
        const char *name;
        const void *ptr;
    } args[] = {{"coef_psi", c_psi}, {"coef_lnne", c_lnne}, {"coef_lnTe", c_lnTe}, {"coef_Br", c_Br},
                {"coef_Bz", c_Bz},   {"coef_Bphi", c_Bphi}, {"vol_coefs", vol_coefs}};
    for (const auto &a : args)
        if (!a.ptr) return fail("torj_plasma_update_from_coefs: %s is NULL", a.name);
    if (n_vol < 2) return fail("torj_plasma_update_from_coefs: n_vol = %d < 2", n_vol);
    torj_plasma_s fresh;  // (no node data: a later profiles-only update is refused)
    if (plasma_from_coefs(&fresh, p->g.nR, p->g.nZ, R1, Rn, Z1, Zn, c_psi, c_lnne, c_lnTe, c_Br, c_Bz, c_Bphi,
                          n_vol, vol_psi1, vol_psin, vol_coefs, psi_prof_max, p->device))
        return -1;
    return plasma_adopt(p, fresh, stream);
}

int torj_plasma_update_profiles(torj_plasma_t p, int n_prof, const double *psi_prof, const double *ne_prof,
                                const double *Te_prof, void *stream) {
    if (!p) return fail("torj_plasma_update_profiles: p is NULL");
    if (!psi_prof) return fail("torj_plasma_update_profiles: psi_prof is NULL");
    if (!ne_prof) return fail("torj_plasma_update_profiles: ne_prof is NULL");
    if (!Te_prof) return fail("torj_plasma_update_profiles: Te_prof is NULL");
    if (n_prof < 2) return fail("torj_plasma_update_profiles: n_prof = %d < 2", n_prof);
    const int nR = p->g.nR, nZ = p->g.nZ;
    if (mirror_sync(p)) return -1;  // after a device-side build: the coefficients and the psi nodes it left there
    torj_plasma_s fresh;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->psi_nodes.empty())
            return fail("torj_plasma_update_profiles: the handle has no psi_norm_data (its equilibrium came as "
                        "coefficients: torj_plasma_create_from_coefs / torj_plasma_update_from_coefs); use "
                        "torj_plasma_update_from_coefs");
        fresh.g = p->g;
        fresh.coef = p->coef;
        fresh.n_vol = p->n_vol, fresh.v1 = p->v1, fresh.vn = p->vn;
        fresh.vol_coef = p->vol_coef;
        fresh.psi_nodes = p->psi_nodes;
    }
    // the ln ne and ln Te slots alone; the equilibrium's four stay as they are
    const size_t nc = (size_t)(nR + 2) * (nZ + 2);
    std::vector<double> c2(nc);
    const double *prof[2] = {ne_prof, Te_prof};
    const int slot[2] = {F_LNNE, F_LNTE};
    for (int f = 0; f < 2; f++) {
        prof2d_coefs(nR, nZ, fresh.psi_nodes.data(), n_prof, psi_prof, prof[f], c2);
        for (size_t k = 0; k < nc; k++) fresh.coef[k * kNF + slot[f]] = c2[k];
    }
    fresh.psi_prof_max = *std::max_element(psi_prof, psi_prof + n_prof);
    return plasma_adopt(p, fresh, stream);
}

// torj_plasma_update with the six 2-D prefilters on the device; all arrays are host arrays
int torj_plasma_update_gpu(torj_plasma_t p, const double *R, const double *Z, const double *psi_norm, int n_prof,
                           const double *psi_prof, const double *ne_prof, const double *Te_prof, const double *Br,
                           const double *Bz, const double *Bphi, int n_eq, const double *eq_psi,
                           const double *eq_vol, void *stream) {
    const char *who = "torj_plasma_update_gpu";
    const NamedPtr args[] = {{"R_coords", R},     {"Z_coords", Z},   {"psi_norm_data", psi_norm}, {"psi_prof", psi_prof},
                             {"ne_prof", ne_prof}, {"Te_prof", Te_prof}, {"Br_data", Br},          {"Bz_data", Bz},
                             {"Bphi_data", Bphi}, {"eqt1d_psi_norm", eq_psi}, {"eqt1d_volume", eq_vol}};
    if (build_checks(p, who, args, sizeof args / sizeof *args, n_prof, &n_eq) || build_device(p, who)) return -1;
    Update1D u;
    update1d_profiles(u, n_prof, psi_prof, ne_prof, Te_prof);
    update1d_full(u, p->g.nR, p->g.nZ, R, Z, n_eq, eq_psi, eq_vol);
    BuildMaps m;
    m.host[0] = psi_norm, m.host[1] = Br, m.host[2] = Bz, m.host[3] = Bphi;
    return plasma_build(p, who, u, m, stream);
}

// ... with psi_norm_data, Br_data, Bz_data, Bphi_data in device memory, read in `stream`'s order
int torj_plasma_update_device(torj_plasma_t p, const double *R, const double *Z, const double *d_psi_norm, int n_prof,
                              const double *psi_prof, const double *ne_prof, const double *Te_prof,
                              const double *d_Br, const double *d_Bz, const double *d_Bphi, int n_eq,
                              const double *eq_psi, const double *eq_vol, void *stream) {
    const char *who = "torj_plasma_update_device";
    const NamedPtr args[] = {{"R_coords", R},     {"Z_coords", Z},   {"psi_norm_data", d_psi_norm}, {"psi_prof", psi_prof},
                             {"ne_prof", ne_prof}, {"Te_prof", Te_prof}, {"Br_data", d_Br},           {"Bz_data", d_Bz},
                             {"Bphi_data", d_Bphi}, {"eqt1d_psi_norm", eq_psi}, {"eqt1d_volume", eq_vol}};
    if (build_checks(p, who, args, sizeof args / sizeof *args, n_prof, &n_eq) || build_device(p, who)) return -1;
    Update1D u;
    update1d_profiles(u, n_prof, psi_prof, ne_prof, Te_prof);
    update1d_full(u, p->g.nR, p->g.nZ, R, Z, n_eq, eq_psi, eq_vol);
    BuildMaps m;
    m.dev[0] = d_psi_norm, m.dev[1] = d_Br, m.dev[2] = d_Bz, m.dev[3] = d_Bphi;
    return plasma_build(p, who, u, m, stream);
}

// torj_plasma_update_profiles with the two 2-D prefilters on the device, from the psi nodes kept there
int torj_plasma_update_profiles_gpu(torj_plasma_t p, int n_prof, const double *psi_prof, const double *ne_prof,
                                    const double *Te_prof, void *stream) {
    const char *who = "torj_plasma_update_profiles_gpu";
    const NamedPtr args[] = {{"psi_prof", psi_prof}, {"ne_prof", ne_prof}, {"Te_prof", Te_prof}};
    if (build_checks(p, who, args, sizeof args / sizeof *args, n_prof, nullptr)) return -1;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        if (p->psi_nodes.empty() && !p->d_psi_valid)
            return fail("%s: the handle has no psi_norm_data (its equilibrium came as coefficients: "
                        "torj_plasma_create_from_coefs / torj_plasma_update_from_coefs); use "
                        "torj_plasma_update_from_coefs", who);
    }
    if (build_device(p, who)) return -1;
    Update1D u;
    update1d_profiles(u, n_prof, psi_prof, ne_prof, Te_prof);
    return plasma_build(p, who, u, BuildMaps{}, stream);
}

int torj_plasma_get_cell_table(torj_plasma_t p, double *out) {
    if (!p) return fail("torj_plasma_get_cell_table: p is NULL");
    if (!out) return fail("torj_plasma_get_cell_table: out is NULL");
    if (!p->d_flags) return fail("torj_plasma_get_cell_table: the handle has no device state yet (no GPU use so far)");
    HIPCK(hipSetDevice(p->device));
    HIPCK(hipStreamSynchronize(p->stream));
    HIPCK(hipMemcpy(out, p->d_cellp, (size_t)(p->g.nR - 1) * (p->g.nZ - 1) * kCellRec * sizeof(double),
                    hipMemcpyDeviceToHost));
    return 0;
}

int torj_plasma_destroy(torj_plasma_t p) {
    if (!p) return 0;
    for (ncclComm_t c : p->comms) (void)ncclCommDestroy(c);
    for (size_t k = 1; k < p->replicas.size(); k++) torj_plasma_destroy(p->replicas[k]);
    if (p->d_coef) (void)hipSetDevice(p->device);
    if (p->stage.sc) (void)hipStreamSynchronize(p->stage.sc);
    if (p->stage.d) (void)hipFree(p->stage.d);
    if (p->stage.h) {
        if (p->stage.h_pinned)
            (void)hipHostFree(p->stage.h);
        else
            free(p->stage.h);
    }
    for (int r = 0; r < 2; r++) {
        if (p->stage.up[r]) (void)hipEventDestroy(p->stage.up[r]);
        if (p->stage.tr[r]) (void)hipEventDestroy(p->stage.tr[r]);
        if (p->stage.dn[r]) (void)hipEventDestroy(p->stage.dn[r]);
    }
    if (p->stage.sc) (void)hipStreamDestroy(p->stage.sc);
    if (p->d_coef) (void)hipFree(p->d_coef);
    if (p->d_cellp) (void)hipFree(p->d_cellp);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    if (p->ev_Nin) (void)hipEventDestroy(p->ev_Nin);
    if (p->ev_Nout) (void)hipEventDestroy(p->ev_Nout);
    if (p->ev_U) (void)hipEventDestroy(p->ev_U);
    if (p->ev_B) (void)hipEventDestroy(p->ev_B);
    if (p->cbuild.d) (void)hipFree(p->cbuild.d);
    if (p->d_psi) (void)hipFree(p->d_psi);
    if (p->sched.d) (void)hipFree(p->sched.d);
    if (p->fit.d) (void)hipFree(p->fit.d);
    if (p->d_flags) (void)hipFree(p->d_flags);
    if (p->chunk.d) (void)hipFree(p->chunk.d);
    for (hipEvent_t e : p->ev_pool) (void)hipEventDestroy(e);
    if (p->ws.d) (void)hipFree(p->ws.d);
    if (p->beams.d) (void)hipFree(p->beams.d);
    if (p->mk.d) (void)hipFree(p->mk.d);
    if (p->split.d) (void)hipFree(p->split.d);
    if (p->batch.d) (void)hipFree(p->batch.d);
    for (int q = 0; q < torj_plasma_s::kRing; q++) {
        if (p->ev_T[q]) (void)hipEventDestroy(p->ev_T[q]);
        if (p->ev_A[q]) (void)hipEventDestroy(p->ev_A[q]);
        if (p->ev_S[q]) (void)hipEventDestroy(p->ev_S[q]);
    }
    if (p->ev_J) (void)hipEventDestroy(p->ev_J);
    if (p->ev_F) (void)hipEventDestroy(p->ev_F);
    if (p->ev_D) (void)hipEventDestroy(p->ev_D);
    if (p->stream2) (void)hipStreamDestroy(p->stream2);
    if (p->streamT) (void)hipStreamDestroy(p->streamT);
    if (p->streamS) (void)hipStreamDestroy(p->streamS);
    if (p->streamD) (void)hipStreamDestroy(p->streamD);
    delete p;
    return 0;
}

int torj_plasma_get_coefs(torj_plasma_t p, int field, double *out) {
    if (!p || field < 0 || field > 5) return fail("bad plasma handle or field index");
    if (mirror_sync(p)) return -1;
    const size_t nodes = (size_t)(p->g.nR + 2) * (p->g.nZ + 2);
    for (size_t k = 0; k < nodes; k++) out[k] = p->coef[k * kNF + kFieldSlot[field]];
    return 0;
}

double torj_plasma_psi_prof_max(torj_plasma_t p) { return p ? p->psi_prof_max : NAN; }

int torj_plasma_volume(torj_plasma_t p, int n, const double *psi, double *vol) {
    if (!p) return fail("bad plasma handle");
    for (int i = 0; i < n; i++) vol[i] = bspl1d_eval(p->vol_coef, p->n_vol, p->v1, p->vn, psi[i]);
    return 0;
}

// (torj_shell_volumes, and torj_make_beams' division of its dP_shell rows)
static void shell_volumes(const torj_plasma_s *p, int n_psi, const double *g, double *dV) {
    for (int j = 0; j + 1 < n_psi; j++)
        dV[j] = bspl1d_eval(p->vol_coef, p->n_vol, p->v1, p->vn, g[j + 1]) -
                bspl1d_eval(p->vol_coef, p->n_vol, p->v1, p->vn, g[j]);
}

int torj_shell_volumes(torj_plasma_t p, int n_psi, const double *g, double *dV) {
    if (!p) return fail("bad plasma handle");
    shell_volumes(p, n_psi, g, dV);
    return 0;
}

void torj_pol_tor_angles_2_vector(double pol, double tor, double N[3]) {
    // IMAS ec_launchers convention: angle_pol = atan2(-k_Z, -k_R), angle_tor = asin(k_phi / k)
    N[0] = -std::cos(pol) * std::cos(tor);
    N[1] = std::sin(tor);
    N[2] = -std::sin(pol) * std::cos(tor);
}

int torj_launch_peripheral_rays(const double x0[3], const double N0[3], double w,
                                double inv_curv, double f, int N_rings, int min_az, int normalize,
                                int *n_rays, double *pos, double *dir, double *weights) {
    if (N_rings < 2) return fail("ArgumentError: N_rings = %d < 2 which is the minimum", N_rings);
    const Rings RG = make_rings(N_rings, min_az, w);
    if (n_rays) *n_rays = RG.total;
    if (!pos) return 0;
    const int n = RG.total;
    const double nn = std::sqrt(N0[0] * N0[0] + N0[1] * N0[1] + N0[2] * N0[2]);
    const double n0[3] = {N0[0] / nn, N0[1] / nn, N0[2] / nn};
    const bool fin = std::isfinite(inv_curv);
    double w0 = w, xw[3] = {0, 0, 0};
    if (fin) {  // :34-47 Gaussian-beam waist
        const double Rc = 1.0 / inv_curv, lam = kC / f;
        const double w4 = w * w * w * w;
        w0 = (lam * std::fabs(Rc) * w) / std::sqrt(lam * lam * Rc * Rc + kPi * kPi * w4);
        const double zw = kPi * kPi * Rc * w4 / (lam * lam * Rc * Rc + kPi * kPi * w4);
        for (int k = 0; k < 3; k++) xw[k] = x0[k] - n0[k] * zw;
    }
    double ec[3] = {1.0, 0.0, -n0[0] / n0[2]};                     // :54-57
    double eu[3] = {-n0[0] * n0[1] / n0[2], n0[2] - n0[0], -n0[1]};  // :61-64
    const double nc = std::sqrt(ec[0] * ec[0] + ec[1] * ec[1] + ec[2] * ec[2]);
    const double nu = std::sqrt(eu[0] * eu[0] + eu[1] * eu[1] + eu[2] * eu[2]);
    for (int k = 0; k < 3; k++) {
        ec[k] /= nc;
        eu[k] /= nu;
    }
    const double sg = inv_curv > 0 ? 1.0 : (inv_curv < 0 ? -1.0 : 0.0);
    int kk = 0;
    for (int i = 0; i < N_rings; i++) {
        const int nt = RG.nth[i];
        for (int j = 0; j < nt; j++) {
            const double th = 2.0 * kPi * (double)j / (double)nt;
            const double chi = RG.r[i] * std::cos(th), ups = RG.r[i] * std::sin(th);
            const int q = kk + j;
            double P[3], D[3];
            for (int k = 0; k < 3; k++) P[k] = chi * ec[k] + ups * eu[k] + x0[k];
            if (fin) {
                for (int k = 0; k < 3; k++) D[k] = w0 / w * (chi * ec[k] + ups * eu[k]) * sg + xw[k];
                if (inv_curv < 0.0)
                    for (int k = 0; k < 3; k++) D[k] -= P[k];
                else
                    for (int k = 0; k < 3; k++) D[k] = -D[k] + P[k];
                const double dn = std::sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
                for (double &c : D) c /= dn;
            } else {
                for (int k = 0; k < 3; k++) D[k] = n0[k];
            }
            for (int k = 0; k < 3; k++) {
                pos[(size_t)k * n + q] = P[k];
                dir[(size_t)k * n + q] = D[k];
            }
            weights[q] = RG.r[i] * RG.rw[i] * (2.0 * kPi / (double)nt);
        }
        kk += nt;
    }
    if (normalize) {  // :125-129
        double s = 0;
        for (int i = 0; i < n; i++) s += weights[i];
        for (int i = 0; i < n; i++) weights[i] /= s;
    } else {
        for (int i = 0; i < n; i++) weights[i] *= 2.0 / (w * w * kPi);
    }
    return 0;
}

int torj_ray_entry(torj_plasma_t p, int n, const double *x0, const double *N0, double omega,
                   int mode, double *xp, double *Np, double *s0, int *status) {
    if (!p) return fail("bad plasma handle");
    if (mode != 1 && mode != -1) return fail("mode must be +1 (X) or -1 (O)");
    if (mirror_sync(p)) return -1;
    const double *coef = p->coef.data();
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        const double a[3] = {x0[i], x0[(size_t)n + i], x0[2 * (size_t)n + i]};
        const double d[3] = {N0[i], N0[(size_t)n + i], N0[2 * (size_t)n + i]};
        double xo[3], No[3];
        status[i] = ray_entry_one(coef, p->g, p->psi_prof_max, a, d, omega, mode, xo, No, s0[i]);
        for (int k = 0; k < 3; k++) {
            xp[(size_t)k * n + i] = xo[k];
            Np[(size_t)k * n + i] = No[k];
        }
    }
    return 0;
}

int torj_eval_plasma(torj_plasma_t p, int n, const double *x, const double *N, double omega,
                     double *out) {
    if (!p) return fail("bad plasma handle");
    if (n <= 0) return 0;
    if (ensure_device(p)) return -1;
    DevBufs B;
    double *dx, *dN, *dout;
    if (B.up(&dx, x, 3 * (size_t)n, p->stream) || B.up(&dN, N, 3 * (size_t)n, p->stream) ||
        B.alloc(&dout, 13 * (size_t)n, true))
        return -1;
    EvalArgs a{};
    a.coef = p->d_coef;
    a.g = p->g;
    a.k = make_consts(omega);
    a.omega = omega;
    a.n = n;
    a.x = dx;
    a.N = dN;
    a.out = dout;
    hipLaunchKernelGGL(k_eval_plasma, dim3(nblocks(n, 256)), dim3(256), 0, p->stream, a);
    HIPCK(hipGetLastError());
    if (ddownload(out, dout, 13 * (size_t)n, p->stream)) return -1;
    HIPCK(hipStreamSynchronize(p->stream));
    return 0;
}

int torj_dispersion(torj_plasma_t p, int n, const double *x, const double *N, double omega,
                    int mode, double *D, double *du, double *alpha) {
    if (!p) return fail("bad plasma handle");
    if (n <= 0) return 0;
    if (ensure_device(p)) return -1;
    if (alpha && ensure_gl_on_device(p->device)) return -1;
    DevBufs B;
    double *dx, *dN, *dD, *ddu, *dal;
    if (B.up(&dx, x, 3 * (size_t)n, p->stream) || B.up(&dN, N, 3 * (size_t)n, p->stream) ||
        B.alloc(&dD, n, D != nullptr) || B.alloc(&ddu, 6 * (size_t)n, du != nullptr) ||
        B.alloc(&dal, n, alpha != nullptr))
        return -1;
    EvalArgs a{};
    a.coef = p->d_coef;
    a.g = p->g;
    a.k = make_consts(omega);
    a.omega = omega;
    a.mode = mode;
    a.n = n;
    a.x = dx;
    a.N = dN;
    a.D = dD;
    a.du = ddu;
    a.alpha = dal;
    if (alpha)
        hipLaunchKernelGGL(k_dispersion<true>, dim3(nblocks(n, 256)), dim3(256), 0, p->stream, a);
    else
        hipLaunchKernelGGL(k_dispersion<false>, dim3(nblocks(n, 256)), dim3(256), 0, p->stream, a);
    HIPCK(hipGetLastError());
    if (ddownload(D, dD, n, p->stream) || ddownload(du, ddu, 6 * (size_t)n, p->stream) ||
        ddownload(alpha, dal, n, p->stream))
        return -1;
    HIPCK(hipStreamSynchronize(p->stream));
    return 0;
}

static int batched_scalar(bool albajar, int n, const double *omega, const double *X,
                          const double *Y, const double *Nabs, const double *Npar,
                          const double *Te, int mode, double *out) {
    if (n <= 0) return 0;
    int dev = 0;
    HIPCK(hipGetDevice(&dev));
    if (albajar && ensure_gl_on_device(dev)) return -1;
    DevBufs B;
    AlbArgs a{};
    a.n = n;
    a.mode = mode;
    double *d[7];
    const double *h[6] = {omega, X, Y, Nabs, Npar, Te};
    for (int k = 0; k < 6; k++) {
        d[k] = nullptr;
        if (h[k] && B.up(&d[k], h[k], n, nullptr)) return -1;
    }
    if (B.alloc(&d[6], n, true)) return -1;
    a.omega = d[0], a.X = d[1], a.Y = d[2], a.Nabs = d[3], a.Npar = d[4], a.Te = d[5];
    a.out = d[6];
    if (albajar)
        hipLaunchKernelGGL(k_albajar, dim3(nblocks(n, 256)), dim3(256), 0, nullptr, a);
    else
        hipLaunchKernelGGL(k_refr, dim3(nblocks(n, 256)), dim3(256), 0, nullptr, a);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(out, d[6], n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int torj_abs_albajar_fast(int n, const double *omega, const double *X, const double *Y,
                          const double *Nabs, const double *Npar, const double *Te, int mode,
                          double *alpha) {
    return batched_scalar(true, n, omega, X, Y, Nabs, Npar, Te, mode, alpha);
}

int torj_alpha_warm(int n, const double *omega, const double *X, const double *Y,
                    const double *Nabs, const double *Npar, const double *Te,
                    const double *inv_dDdN, int mode, int iwarm, double *alpha, double *Nperp2) {
    if (n <= 0) return 0;
    if (iwarm != 1 && iwarm != 3) return fail("iwarm must be 1 or 3");
    if (mode != 1 && mode != -1) return fail("mode must be +1 (X) or -1 (O)");
    DevBufs B;
    AlbArgs a{};
    a.n = n;
    a.mode = mode;
    a.iwarm = iwarm;
    double *d[9];
    const double *h[7] = {omega, X, Y, Nabs, Npar, Te, inv_dDdN};
    for (int k = 0; k < 7; k++) {
        if (!h[k]) return fail("torj_alpha_warm: every input array is required");
        if (B.up(&d[k], h[k], n, nullptr)) return -1;
    }
    if (B.alloc(&d[7], n, true) || B.alloc(&d[8], 2 * (size_t)n, true)) return -1;
    a.omega = d[0], a.X = d[1], a.Y = d[2], a.Nabs = d[3], a.Npar = d[4], a.Te = d[5];
    a.inv = d[6], a.out = d[7], a.n2 = d[8];
    hipLaunchKernelGGL(k_alpha_warm, dim3(nblocks(n, 64)), dim3(64), 0, nullptr, a);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(alpha, d[7], n * sizeof(double), hipMemcpyDeviceToHost));
    if (Nperp2) HIPCK(hipMemcpy(Nperp2, d[8], 2 * n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int torj_refractive_index_sq(int n, const double *X, const double *Y, const double *Npar, int mode,
                             double *out) {
    return batched_scalar(false, n, nullptr, X, Y, nullptr, Npar, nullptr, mode, out);
}

int torj_ray_entry_device(torj_plasma_t p, int n, const double *x0, const double *N0, double omega,
                          int mode, double *xp, double *Np, double *s0, int *status, void *stream) {
    if (!p) return fail("bad plasma handle");
    if (mode != 1 && mode != -1) return fail("mode must be +1 (X) or -1 (O)");
    if (n <= 0) return 0;
    if (ensure_device(p)) return -1;
    EntryArgs a{p->d_coef, p->g, p->psi_prof_max, omega, mode, n, x0, N0, xp, Np, s0, status};
    hipLaunchKernelGGL(k_ray_entry, dim3(nblocks(n, 64)), dim3(64), 0, (hipStream_t)stream, a);
    HIPCK(hipGetLastError());
    return 0;
}

int torj_ray_entry_gpu(torj_plasma_t p, int n, const double *x0, const double *N0, double omega,
                       int mode, double *xp, double *Np, double *s0, int *status) {
    if (!p) return fail("bad plasma handle");
    if (n <= 0) return 0;
    EntryIO io{};
    io.n = n, io.x0 = x0, io.N0 = N0, io.xp = xp, io.Np = Np, io.s0 = s0, io.status = status;
    return entry_staged(p, io, [&](const EntryIO &d, hipStream_t s) {
        return torj_ray_entry_device(p, d.n, d.x0, d.N0, omega, mode, d.xp, d.Np, d.s0, d.status, s);
    });
}

int torj_trace_device(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
                      const double *N0, const double *weights, int n_psi, const double *grid,
                      double *state, int *status, int *steps, double *dP, double *Pdep,
                      double *traj, uint64_t *counters, void *stream) {
    return torj_trace_device_ex(p, cfg, n, x0, N0, weights, n_psi, grid, nullptr, nullptr, state,
                                status, steps, dP, Pdep, traj, counters, stream);
}

int torj_trace_device_ex(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
                         const double *N0, const double *weights, int n_psi, const double *grid,
                         const double *x_launch, const double *s0, double *state, int *status,
                         int *steps, double *dP, double *Pdep, double *traj, uint64_t *counters,
                         void *stream) {
    RayIO io{};
    io.n = n, io.x0 = x0, io.N0 = N0, io.weights = weights, io.psi_grid = grid, io.x_launch = x_launch, io.s0 = s0;
    io.state = state, io.status = status, io.steps = steps, io.dP_shell = dP, io.P_dep = Pdep, io.traj = traj;
    io.counters = counters;
    return trace_device(p, cfg, io, n_psi, stream);
}

// ---- many beams of differing frequency and mode in one launch (beams_plan, torj_k_beams.hpp),
// and through differing plasmas (`ps`: beams_plasmas_plan) ----
}  // extern "C"

// host pointers, synchronous, checked
static int beams_host_entry(torj_plasma_t p, const PlasmaSel *ps, const torj_trace_cfg *cfg, const BeamTables &bt,
                            const RayIO &caller, int n_psi) {
    if (!p || !cfg) return fail("bad plasma handle or cfg");
    const bool depo = n_psi >= 2 && caller.psi_grid;
    BeamsPlasmasPlan pp;  // argument errors before any device work (the device form repeats them on its pointers)
    LaunchPtrs has = launch_ptrs(caller);
    has.grid = has.dP = depo;  // host arrays: the device form gets both from trace_staged exactly when depo
    if (beams_any_plan(pp, p, ps, *cfg, bt, n_psi, has) || (depo && grid_increasing(n_psi, caller.psi_grid))) return -1;
    RayIO h = caller;
    h.n = bt.beam_off[bt.n_beams];
    if (h.n == 0) {
        if (h.dP_shell) std::fill(h.dP_shell, h.dP_shell + dP_rows(bt.n_beams, n_psi), 0.0);
        return 0;
    }
    return trace_staged(p, cfg, h, bt.n_beams, n_psi, [&](const RayIO &d, int n_psi_d, hipStream_t s) {
        return beams_trace_device(p, ps, cfg, bt, d, n_psi_d, s);
    });
}

// the ray entry's argument errors: the tables', then the arrays'; no HIP call
static int entry_beams_check(torj_plasma_t p, const PlasmaSel *ps, const BeamTables &bt, const EntryIO &io) {
    if (!p) return fail("bad plasma handle");
    if (ps && beams_plasmas_check(ps->n, (const void *const *)ps->list, ps->beam_plasma, p->device, kHandleView))
        return -1;
    if (beams_tables_check(bt.n_beams, bt.beam_off, bt.omega, bt.mode)) return -1;
    if (ps && beam_plasma_check(ps->n, ps->beam_plasma, bt.n_beams)) return -1;
    if (!io.x0 || !io.N0 || !io.xp || !io.Np || !io.s0 || !io.status)
        return fail("x0, N0, x_plasma, N_plasma, s0, status required");
    return 0;
}

static int entry_beams_device(torj_plasma_t p, const PlasmaSel *ps, const BeamTables &bt, const EntryIO &io,
                              void *stream) {
    if (entry_beams_check(p, ps, bt, io)) return -1;
    const int n_beams = bt.n_beams, n = bt.beam_off[n_beams];
    if (n == 0) return 0;
    if (ensure_devices(p, ps)) return -1;
    const dim3 grd(nblocks(n, 64)), blk(64);
    EntryArgs a{p->d_coef, p->g, p->psi_prof_max, 0.0, 0, n, io.x0, io.N0, io.xp, io.Np, io.s0, io.status};
    std::vector<PlasmaRec> plasmas;
    std::vector<int> beam_pl;
    if (ps) {
        beam_pl.assign(ps->beam_plasma, ps->beam_plasma + n_beams);
        for (int j = 0; j < ps->n; j++) plasmas.push_back(kHandleView.rec(ps->list[j]));
    }
    const BeamRec *d_beams;
    const PlasmaRec *d_plasmas;
    const int *d_beam_pl;
    if (beams_upload(p, beams_records(n_beams, bt.beam_off, bt.omega, bt.mode), {}, plasmas, beam_pl,
                     (hipStream_t)stream, &d_beams, nullptr, &d_plasmas, &d_beam_pl))
        return -1;
    if (ps)
        hipLaunchKernelGGL(k_ray_entry_beams, grd, blk, 0, (hipStream_t)stream, a, d_beams, n_beams, d_plasmas,
                           d_beam_pl);
    else
        hipLaunchKernelGGL(k_ray_entry_beams, grd, blk, 0, (hipStream_t)stream, a, d_beams, n_beams);
    HIPCK(hipGetLastError());
    return 0;
}

static int entry_beams_host(torj_plasma_t p, const PlasmaSel *ps, const BeamTables &bt, const EntryIO &caller) {
    if (entry_beams_check(p, ps, bt, caller)) return -1;
    EntryIO h = caller;
    h.n = bt.beam_off[bt.n_beams];
    if (h.n == 0) return 0;
    return entry_staged(p, h, [&](const EntryIO &d, hipStream_t s) { return entry_beams_device(p, ps, bt, d, s); });
}

// ---- make_beams as one call (torj_make_beams): the launchers' fans on the host, the ray entry
// of all rays on the GPU, the rays that entered closed up (beams_compact, k_rays_gather), one
// multi-beam trace of those, its outputs back in launched order (k_rays_scatter) ----
struct BeamFans {  // every launcher's rays, concatenated in launcher order, and the beams' tables
    std::vector<int> off, mode, beam_pl;  // n_beams + 1, n_beams, n_beams
    std::vector<double> omega;            // n_beams
    std::vector<double> pos, dir, w;      // 3 x n, 3 x n, n, component-major over all n rays
};

// make_beam's launch per launcher (src/solve.jl:211-216) by the functions the single calls use;
// count_only stops at the offsets
static int make_beams_fans(BeamFans &F, int n_beams, const torj_launcher *la, int N_rings, int min_az,
                           bool count_only) {
    F = BeamFans{};
    F.off.assign(1, 0);
    std::vector<double> x0(3 * (size_t)n_beams), N0(3 * (size_t)n_beams);
    for (int b = 0; b < n_beams; b++) {
        const torj_launcher &l = la[b];
        torj_pol_tor_angles_2_vector(l.steering_angle_pol, l.steering_angle_tor, &N0[3 * b]);
        x0[3 * b] = l.r * std::cos(l.phi), x0[3 * b + 1] = l.r * std::sin(l.phi), x0[3 * b + 2] = l.z;
        int nb = 0;
        if (torj_launch_peripheral_rays(&x0[3 * b], &N0[3 * b], l.spot_size, l.inverse_curvature_radius, l.f, N_rings,
                                        min_az, 1, &nb, nullptr, nullptr, nullptr))
            return -1;
        if ((long long)F.off[b] + nb > 0x7fffffffll / 8)
            return fail("torj_make_beams: launchers 0..%d launch more than %d rays", b, 0x7fffffff / 8);
        F.off.push_back(F.off[b] + nb);
        F.omega.push_back(2.0 * kPi * l.f);
        F.mode.push_back(l.mode);
        F.beam_pl.push_back(l.plasma);
    }
    if (count_only) return 0;
    const size_t n = (size_t)F.off[n_beams];
    F.pos.resize(3 * n), F.dir.resize(3 * n), F.w.resize(n);
    std::vector<double> pos, dir;
    for (int b = 0; b < n_beams; b++) {
        const torj_launcher &l = la[b];
        const size_t lo = (size_t)F.off[b], nb = (size_t)F.off[b + 1] - lo;
        pos.resize(3 * nb), dir.resize(3 * nb);
        if (torj_launch_peripheral_rays(&x0[3 * b], &N0[3 * b], l.spot_size, l.inverse_curvature_radius, l.f, N_rings,
                                        min_az, 1, nullptr, pos.data(), dir.data(), F.w.data() + lo))
            return -1;
        for (int c = 0; c < 3; c++) {
            std::copy(pos.begin() + c * nb, pos.begin() + (c + 1) * nb, F.pos.begin() + c * n + lo);
            std::copy(dir.begin() + c * nb, dir.begin() + (c + 1) * nb, F.dir.begin() + c * n + lo);
        }
    }
    return 0;
}

// the device part, enqueued: entry, compaction, trace, and every output the caller asked for.
// est: the n entry statuses; dP: n_beams rows of n_psi + 1 (dP_shell as torj_trace_beams gives
// it); idx: the gather index and its inverse, the caller's because the stream copies from it
static int make_beams_enqueue(torj_plasma_t p, const PlasmaSel *ps, const torj_trace_cfg *cfg, const BeamFans &F,
                              int n_psi, const double *grid, const torj_beams_rays &out, std::vector<int> &est,
                              BeamsCompact &bc, std::vector<double> &dP, std::vector<int> &idx) {
    const int B = (int)F.omega.size(), n = F.off[B];
    const size_t N = (size_t)n, rows = dP_rows(B, n_psi);
    const int n_save = out.traj && cfg->traj_stride > 0 ? cfg->n_steps / cfg->traj_stride : 0;
    est.assign(N, 0);  // (n >= 2 n_beams: every ring of a fan has a ray)
    dP.assign(rows, 0.0);
    if (ensure_devices(p, ps)) return -1;
    hipStream_t s = p->stream;
    // one grow-only buffer of the handle holds every array of the call: the kept rays' arrays
    // at the launched size too, so that it is sized before the entry has run
    size_t bytes = 0;
    auto take = [&](size_t b) {
        const size_t at = bytes;
        bytes += (b + 255) & ~(size_t)255;
        return at;
    };
    const size_t D = sizeof(double), I = sizeof(int), T = (size_t)n_save * 5 * N * D;
    const size_t o_pos = take(3 * N * D), o_dir = take(3 * N * D), o_w = take(N * D), o_xp = take(3 * N * D),
                 o_Np = take(3 * N * D), o_s0 = take(N * D), o_state = take(7 * N * D), o_Pdep = take(N * D),
                 o_traj = take(T), o_pos_c = take(3 * N * D), o_w_c = take(N * D), o_xp_c = take(3 * N * D),
                 o_Np_c = take(3 * N * D), o_s0_c = take(N * D), o_state_c = take(7 * N * D), o_Pdep_c = take(N * D),
                 o_traj_c = take(T), o_grid = take((size_t)n_psi * D), o_dP = take(rows * D), o_est = take(N * I),
                 o_status = take(N * I), o_steps = take(N * I), o_status_c = take(N * I), o_steps_c = take(N * I),
                 o_idx = take(2 * N * I);
    if (ensure_buf(p, p->mk, bytes)) return -1;
    char *base = (char *)p->mk.d;
    auto dd = [&](size_t o) { return (double *)(base + o); };
    auto di = [&](size_t o) { return (int *)(base + o); };
    HIPCK(hipMemcpyAsync(dd(o_pos), F.pos.data(), 3 * N * D, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(dd(o_dir), F.dir.data(), 3 * N * D, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(dd(o_w), F.w.data(), N * D, hipMemcpyHostToDevice, s));
    HIPCK(hipMemcpyAsync(dd(o_grid), grid, (size_t)n_psi * D, hipMemcpyHostToDevice, s));
    HIPCK(hipMemsetAsync(dd(o_dP), 0, rows * D, s));
    const BeamTables bt = {B, F.off.data(), F.omega.data(), F.mode.data()};
    EntryIO e{};
    e.n = n, e.x0 = dd(o_pos), e.N0 = dd(o_dir), e.xp = dd(o_xp), e.Np = dd(o_Np), e.s0 = dd(o_s0), e.status = di(o_est);
    if (entry_beams_device(p, ps, bt, e, s)) return -1;
    // (the one read-back ahead of the trace: 4 n bytes)
    HIPCK(hipMemcpyAsync(est.data(), e.status, N * I, hipMemcpyDeviceToHost, s));
    HIPCK(hipStreamSynchronize(s));
    beams_compact(bc, B, F.off.data(), est.data());
    const int m = bc.beam_off[B];
    idx.assign(2 * N, -1);  // the gather index (m of n entries used), then its inverse
    for (int k = 0; k < m; k++) idx[k] = bc.gather[k], idx[N + bc.gather[k]] = k;
    HIPCK(hipMemcpyAsync(di(o_idx), idx.data(), 2 * N * I, hipMemcpyHostToDevice, s));
    if (m > 0) {
        const RaysGatherArgs g = {n,           m,         di(o_idx),   dd(o_pos),  dd(o_w),    dd(o_xp),   dd(o_Np),
                                  dd(o_s0),    dd(o_pos_c), dd(o_w_c), dd(o_xp_c), dd(o_Np_c), dd(o_s0_c)};
        hipLaunchKernelGGL(k_rays_gather, dim3(nblocks(m, 64)), dim3(64), 0, s, g);
        HIPCK(hipGetLastError());
    }
    RayIO io{};
    io.x0 = dd(o_xp_c), io.N0 = dd(o_Np_c), io.weights = dd(o_w_c), io.psi_grid = dd(o_grid);
    io.x_launch = dd(o_pos_c), io.s0 = dd(o_s0_c), io.state = dd(o_state_c), io.status = di(o_status_c);
    io.steps = di(o_steps_c), io.dP_shell = dd(o_dP), io.P_dep = dd(o_Pdep_c), io.traj = n_save ? dd(o_traj_c) : nullptr;
    const BeamTables btc = {B, bc.beam_off.data(), F.omega.data(), F.mode.data()};
    if (beams_trace_device(p, ps, cfg, btc, io, n_psi, s)) return -1;
    const RaysScatterArgs sc = {n,           m,           n_save,        di(o_idx) + N,    di(o_est),  dd(o_state_c),
                                dd(o_Pdep_c), dd(o_traj_c), di(o_status_c), di(o_steps_c), dd(o_state), dd(o_Pdep),
                                dd(o_traj),  di(o_status), di(o_steps)};
    hipLaunchKernelGGL(k_rays_scatter, dim3(nblocks(n, 64), 1 + std::min(n_save, 1024)), dim3(64), 0, s, sc);
    HIPCK(hipGetLastError());
    if (ddownload(out.x_plasma, dd(o_xp), 3 * N, s) || ddownload(out.N_plasma, dd(o_Np), 3 * N, s) ||
        ddownload(out.s0, dd(o_s0), N, s) || ddownload(out.state, dd(o_state), 7 * N, s) ||
        ddownload(out.status, di(o_status), N, s) || ddownload(out.steps, di(o_steps), N, s) ||
        ddownload(out.P_dep, dd(o_Pdep), N, s) || ddownload(dP.data(), dd(o_dP), rows, s))
        return -1;
    if (n_save && ddownload(out.traj, dd(o_traj), (size_t)n_save * 5 * N, s)) return -1;
    return torj_trace_check(p, s);
}

// ... and waited for.  A refusal or failure half-way (the workspace budget, a failed launch or
// copy) leaves copies from and to host arrays of this call in the stream: they end before those go
static int make_beams_device(torj_plasma_t p, const PlasmaSel *ps, const torj_trace_cfg *cfg, const BeamFans &F,
                             int n_psi, const double *grid, const torj_beams_rays &out, std::vector<int> &est,
                             BeamsCompact &bc, std::vector<double> &dP) {
    std::vector<int> idx;
    const int rc = make_beams_enqueue(p, ps, cfg, F, n_psi, grid, out, est, bc, dP, idx);
    if (rc && p->stream) (void)hipStreamSynchronize(p->stream);  // (the error text stays the failure's)
    return rc;
}

extern "C" {

int torj_trace_beams_device(torj_plasma_t p, const torj_trace_cfg *cfg, int n_beams, const int *beam_off,
                            const double *omega, const int *mode, const double *x0, const double *N0,
                            const double *weights, int n_psi, const double *grid, const double *x_launch,
                            const double *s0, double *state, int *status, int *steps, double *dP,
                            double *Pdep, double *traj, uint64_t *counters, void *stream) {
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    RayIO io{};
    io.x0 = x0, io.N0 = N0, io.weights = weights, io.psi_grid = grid, io.x_launch = x_launch, io.s0 = s0;
    io.state = state, io.status = status, io.steps = steps, io.dP_shell = dP, io.P_dep = Pdep, io.traj = traj;
    io.counters = counters;
    return beams_trace_device(p, nullptr, cfg, bt, io, n_psi, stream);
}

int torj_trace_beams(torj_plasma_t p, const torj_trace_cfg *cfg, int n_beams, const int *beam_off,
                     const double *omega, const int *mode, const double *x0, const double *N0,
                     const double *weights, int n_psi, const double *grid, const double *x_launch,
                     const double *s0, double *state, int *status, int *steps, double *dP, double *Pdep,
                     double *traj) {
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    RayIO io{};
    io.x0 = x0, io.N0 = N0, io.weights = weights, io.psi_grid = grid, io.x_launch = x_launch, io.s0 = s0;
    io.state = state, io.status = status, io.steps = steps, io.dP_shell = dP, io.P_dep = Pdep, io.traj = traj;
    return beams_host_entry(p, nullptr, cfg, bt, io, n_psi);
}

int torj_ray_entry_beams_device(torj_plasma_t p, int n_beams, const int *beam_off, const double *omega,
                                const int *mode, const double *x0, const double *N0, double *xp, double *Np,
                                double *s0, int *status, void *stream) {
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    EntryIO io{};
    io.x0 = x0, io.N0 = N0, io.xp = xp, io.Np = Np, io.s0 = s0, io.status = status;
    return entry_beams_device(p, nullptr, bt, io, stream);
}

int torj_ray_entry_beams_gpu(torj_plasma_t p, int n_beams, const int *beam_off, const double *omega,
                             const int *mode, const double *x0, const double *N0, double *xp, double *Np,
                             double *s0, int *status) {
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    EntryIO io{};
    io.x0 = x0, io.N0 = N0, io.xp = xp, io.Np = Np, io.s0 = s0, io.status = status;
    return entry_beams_host(p, nullptr, bt, io);
}

// beam b through plasmas[beam_plasma[b]]; p is the launch's handle (stream, scratch, flags, knobs)
int torj_trace_beams_plasmas_device(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                                    const int *beam_plasma, const torj_trace_cfg *cfg, int n_beams,
                                    const int *beam_off, const double *omega, const int *mode, const double *x0,
                                    const double *N0, const double *weights, int n_psi, const double *grid,
                                    const double *x_launch, const double *s0, double *state, int *status,
                                    int *steps, double *dP, double *Pdep, double *traj, uint64_t *counters,
                                    void *stream) {
    const PlasmaSel ps = {n_plasmas, plasmas, beam_plasma};
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    RayIO io{};
    io.x0 = x0, io.N0 = N0, io.weights = weights, io.psi_grid = grid, io.x_launch = x_launch, io.s0 = s0;
    io.state = state, io.status = status, io.steps = steps, io.dP_shell = dP, io.P_dep = Pdep, io.traj = traj;
    io.counters = counters;
    return beams_trace_device(p, &ps, cfg, bt, io, n_psi, stream);
}

int torj_trace_beams_plasmas(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas, const int *beam_plasma,
                             const torj_trace_cfg *cfg, int n_beams, const int *beam_off, const double *omega,
                             const int *mode, const double *x0, const double *N0, const double *weights, int n_psi,
                             const double *grid, const double *x_launch, const double *s0, double *state,
                             int *status, int *steps, double *dP, double *Pdep, double *traj) {
    const PlasmaSel ps = {n_plasmas, plasmas, beam_plasma};
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    RayIO io{};
    io.x0 = x0, io.N0 = N0, io.weights = weights, io.psi_grid = grid, io.x_launch = x_launch, io.s0 = s0;
    io.state = state, io.status = status, io.steps = steps, io.dP_shell = dP, io.P_dep = Pdep, io.traj = traj;
    return beams_host_entry(p, &ps, cfg, bt, io, n_psi);
}

// ---- ray profiles: one row of TORJ_PROF_NCOL columns per saved point of every ray (profile_device) ----
static_assert(kProfCols == TORJ_PROF_NCOL, "the kernels' row width is the header's");

int torj_ray_profile_device(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas, const int *beam_plasma,
                            const torj_trace_cfg *cfg, int n_beams, const int *beam_off, const double *omega,
                            const int *mode, const double *x0, const double *N0, const double *s0, int n_rows,
                            double *prof, double *state, int *status, int *steps, void *stream) {
    const PlasmaSel ps = {n_plasmas, plasmas, beam_plasma};
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    RayIO io{};
    io.x0 = x0, io.N0 = N0, io.s0 = s0, io.state = state, io.status = status, io.steps = steps;
    return profile_device(p, n_plasmas == 0 && !plasmas ? nullptr : &ps, cfg, bt, io, n_rows, prof, stream);
}

// host pointers, synchronous, checked: the table lives on the device for the call
int torj_ray_profile(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas, const int *beam_plasma,
                     const torj_trace_cfg *cfg, int n_beams, const int *beam_off, const double *omega,
                     const int *mode, const double *x0, const double *N0, const double *s0, int n_rows,
                     double *prof, double *state, int *status, int *steps) {
    const PlasmaSel sel = {n_plasmas, plasmas, beam_plasma};
    const PlasmaSel *ps = n_plasmas == 0 && !plasmas ? nullptr : &sel;
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    RayIO h{};
    h.x0 = x0, h.N0 = N0, h.s0 = s0, h.state = state, h.status = status, h.steps = steps;
    {
        BeamsPlasmasPlan pp;  // argument errors before any device work (the device form repeats them on its pointers)
        if (profile_plan(pp, p, ps, cfg, bt, h, n_rows, prof)) return -1;
    }
    const size_t n = (size_t)beam_off[n_beams], cells = (size_t)n_rows * TORJ_PROF_NCOL * n;
    if (n == 0) return 0;
    if (ensure_device(p)) return -1;
    hipStream_t s = p->stream;
    DevBufs B;
    RayIO d{};
    if (B.up(&d.x0, h.x0, 3 * n, s) || B.up(&d.N0, h.N0, 3 * n, s) || B.up(&d.s0, h.s0, n, s)) return -1;
    if (B.alloc(&d.state, 7 * n, h.state != nullptr) || B.alloc(&d.status, n, h.status != nullptr) ||
        B.alloc(&d.steps, n, h.steps != nullptr))
        return -1;
    double *d_prof = nullptr;
    if (hipMalloc(&d_prof, cells * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        return fail("torj_ray_profile: no device memory for the table of %zu bytes (%d rows x %d columns x %zu rays)",
                    cells * sizeof(double), n_rows, TORJ_PROF_NCOL, n);
    }
    B.track(d_prof);
    if (profile_device(p, ps, cfg, bt, d, n_rows, d_prof, s)) return -1;
    if (ddownload(prof, d_prof, cells, s) || ddownload(h.state, d.state, 7 * n, s) ||
        ddownload(h.status, d.status, n, s) || ddownload(h.steps, d.steps, n, s))
        return -1;
    return torj_trace_check(p, s);
}

int torj_ray_entry_beams_plasmas_device(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                                        const int *beam_plasma, int n_beams, const int *beam_off,
                                        const double *omega, const int *mode, const double *x0, const double *N0,
                                        double *xp, double *Np, double *s0, int *status, void *stream) {
    const PlasmaSel ps = {n_plasmas, plasmas, beam_plasma};
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    EntryIO io{};
    io.x0 = x0, io.N0 = N0, io.xp = xp, io.Np = Np, io.s0 = s0, io.status = status;
    return entry_beams_device(p, &ps, bt, io, stream);
}

int torj_ray_entry_beams_plasmas_gpu(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                                     const int *beam_plasma, int n_beams, const int *beam_off, const double *omega,
                                     const int *mode, const double *x0, const double *N0, double *xp, double *Np,
                                     double *s0, int *status) {
    const PlasmaSel ps = {n_plasmas, plasmas, beam_plasma};
    const BeamTables bt = {n_beams, beam_off, omega, mode};
    EntryIO io{};
    io.x0 = x0, io.N0 = N0, io.xp = xp, io.Np = Np, io.s0 = s0, io.status = status;
    return entry_beams_host(p, &ps, bt, io);
}

int torj_make_beams(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas, int n_beams,
                    const torj_launcher *launchers, int N_rings, int min_azimuthal_points, const torj_trace_cfg *cfg,
                    int n_psi, const double *grid, double *dP_dV, torj_beam_result *res, int *ray_off,
                    const torj_beams_rays *rays) {
    const bool count_only = !dP_dV && !res && !rays && ray_off;
    if (!launchers) return fail("torj_make_beams: launchers is NULL");
    if (n_beams < 1 || n_beams > kMaxBeams) return fail("torj_make_beams: n_beams must be 1..%d", kMaxBeams);
    if (!count_only) {
        if (!p) return fail("torj_make_beams: p is NULL");
        if (!cfg) return fail("torj_make_beams: cfg is NULL");
        if (!grid) return fail("torj_make_beams: psi_dP_dV is NULL");
        if (n_psi < 2) return fail("torj_make_beams: n_psi must be >= 2");
        if (n_plasmas < 0 || (n_plasmas == 0) != (plasmas == nullptr))
            return fail("torj_make_beams: n_plasmas = %d with plasmas %s (n_plasmas == 0 and plasmas == NULL: every "
                        "beam through p; else n_plasmas >= 1 listed handles)",
                        n_plasmas, plasmas ? "given" : "NULL");
    }
    for (int b = 0; b < n_beams; b++) {
        const torj_launcher &l = launchers[b];
        if (!(l.f > 0) || !std::isfinite(l.f)) return fail("torj_make_beams: launchers[%d].f must be finite and > 0", b);
        if (l.mode != 1 && l.mode != -1) return fail("torj_make_beams: launchers[%d].mode must be +1 (X) or -1 (O)", b);
        if (!count_only && n_plasmas > 0 && (l.plasma < 0 || l.plasma >= n_plasmas))
            return fail("torj_make_beams: launchers[%d].plasma = %d is outside 0..%d (n_plasmas = %d)", b, l.plasma,
                        n_plasmas - 1, n_plasmas);
    }
    BeamFans F;
    if (make_beams_fans(F, n_beams, launchers, N_rings, min_azimuthal_points, count_only)) return -1;
    if (ray_off) std::copy(F.off.begin(), F.off.end(), ray_off);
    if (count_only) return 0;
    // the trace's own refusals, on the launched tables (the kept rays' are a subset): no HIP call yet
    const PlasmaSel sel = {n_plasmas, plasmas, F.beam_pl.data()}, *ps = n_plasmas > 0 ? &sel : nullptr;
    const torj_beams_rays out = rays ? *rays : torj_beams_rays{};
    {
        const BeamTables bt = {n_beams, F.off.data(), F.omega.data(), F.mode.data()};
        const LaunchPtrs has = {true, true, true, true, true, out.traj != nullptr};
        BeamsPlasmasPlan pp;
        if (beams_any_plan(pp, p, ps, *cfg, bt, n_psi, has) || grid_increasing(n_psi, grid)) return -1;
    }
    std::vector<int> est;
    std::vector<double> dP;
    BeamsCompact bc;
    if (make_beams_device(p, ps, cfg, F, n_psi, grid, out, est, bc, dP)) return -1;
    const size_t n = (size_t)F.off[n_beams];
    if (out.pos) std::copy(F.pos.begin(), F.pos.end(), out.pos);
    if (out.dir) std::copy(F.dir.begin(), F.dir.end(), out.dir);
    if (out.weights) std::copy(F.w.begin(), F.w.end(), out.weights);
    if (out.entry_status) std::copy(est.begin(), est.begin() + n, out.entry_status);
    // row b over the shell volumes of beam b's plasma (torj_shell_volumes' function), each plasma's once
    std::vector<std::vector<double>> dV(ps ? n_plasmas : 1);
    for (int b = 0; b < n_beams; b++) {
        const double *row = dP.data() + (size_t)b * (size_t)(n_psi + 1);
        if (dP_dV) {
            const int j = ps ? F.beam_pl[b] : 0;
            if (dV[j].empty()) {
                dV[j].resize((size_t)n_psi - 1);
                shell_volumes(ps ? plasmas[j] : p, n_psi, grid, dV[j].data());
            }
            double *o = dP_dV + (size_t)b * (size_t)n_psi;
            for (int k = 0; k + 1 < n_psi; k++) o[k] = row[k] / dV[j][k];
            o[n_psi - 1] = 0.0;
        }
        if (res) {
            double w_ok = 0.0;
            for (int i = F.off[b]; i < F.off[b + 1]; i++)
                if (est[i] == TORJ_RAY_OK) w_ok += F.w[i];
            res[b] = torj_beam_result{F.off[b + 1] - F.off[b], bc.n_ok[b], bc.first_bad_ray[b], bc.first_bad_status[b],
                                      w_ok, row[n_psi]};
        }
    }
    return 0;
}

int torj_power_deposition_profile(torj_plasma_t p, int n_rays, const int *n_points, const double *s,
                                  const double *x, const double *dP_ds, int n_psi,
                                  const double *grid, double *dP_dV, double *P) {
    if (!p) return fail("bad plasma handle");
    if (n_rays < 0 || n_psi < 2 || !grid) return fail("power_deposition_profile: n_rays >= 0, n_psi >= 2 needed");
    if (n_rays == 0) return 0;
    if (!n_points || !s || !x || !dP_ds || !dP_dV || !P) return fail("power_deposition_profile: null argument");
    if (grid_increasing(n_psi, grid)) return -1;
    std::vector<long> off(n_rays);
    long tot = 0;
    int rows = 0;
    for (int r = 0; r < n_rays; r++) {
        // Dierckx.Spline1D(s, y, k = 3) needs m > k points with strictly
        // increasing s (FITPACK curfit's input check)
        if (n_points[r] < 4) return fail("power_deposition_profile: ray %d has %d points (need >= 4)", r, n_points[r]);
        for (int j = 1; j < n_points[r]; j++)
            if (!(s[tot + j] > s[tot + j - 1]))
                return fail("power_deposition_profile: s must be strictly increasing (ray %d, point %d)", r, j);
        off[r] = tot;
        tot += n_points[r];
        rows = std::max(rows, n_points[r]);
    }
    if (ensure_device(p)) return -1;
    hipStream_t st = p->stream;
    const size_t N = (size_t)n_rays, L = (size_t)n_psi;
    const FitLayout lay = fit_layout(N, (size_t)rows, L, true);  // the trace's workspace, arc lengths stored
    DevBufs B;
    double *d_s, *d_x, *d_dp, *d_grid, *d_Pr;
    int *d_np;
    long *d_off;
    char *d_fit;
    if (B.up(&d_s, s, (size_t)tot, st) || B.up(&d_x, x, 3 * (size_t)tot, st) ||
        B.up(&d_dp, dP_ds, (size_t)tot, st) || B.up(&d_grid, grid, L, st) ||
        B.up(&d_np, n_points, N, st) || B.up(&d_off, off.data(), N, st) ||
        B.alloc(&d_fit, lay.bytes(), true) || B.alloc(&d_Pr, N, true))
        return -1;
    FitArgs fa{};
    fit_point(lay, d_fit, fa, nullptr);
    fa.coef = p->d_coef;
    fa.g = p->g;
    fa.n = n_rays;
    fa.n_psi = n_psi;
    fa.grid = d_grid;
    fa.npts = d_np;
    fa.steps = d_np;
    fa.Pray = d_Pr;
    if (fit_zero(fa, st)) return -1;
    hipLaunchKernelGGL(k_profile_samples, dim3(nblocks(n_rays, 64)), dim3(64), 0, st, fa, d_off, d_s, d_x,
                       (size_t)tot, d_dp);
    hipLaunchKernelGGL(k_fit_profile, dim3(nblocks(n_rays, 64)), dim3(64), fit_grid_lds(n_psi), st, fa);
    HIPCK(hipGetLastError());
    std::vector<double> dPs(L * N);
    std::vector<int> kstar(N);
    if (ddownload(dPs.data(), fa.dPs, (L - 1) * N, st) || ddownload(kstar.data(), fa.kstar, N, st) ||
        ddownload(P, d_Pr, N, st))
        return -1;
    HIPCK(hipStreamSynchronize(st));
    // dP_dV[j] = dP_j / (V(psi_{j+1}) - V(psi_j)) above the break shell, 0 below it
    // and at the last boundary (src/plasma.jl:141)
    std::vector<double> dV(L - 1);
    if (torj_shell_volumes(p, n_psi, grid, dV.data())) return -1;
    for (size_t r = 0; r < N; r++) {
        double *row = dP_dV + r * L;
        for (size_t j = 0; j < L; j++)
            row[j] = (j + 1 < L && (int)j > kstar[r]) ? dPs[j * N + r] / dV[j] : 0.0;
    }
    return 0;
}

int torj_timing(torj_plasma_t p, int enable) {
    if (!p) return fail("bad plasma handle");
    std::lock_guard<std::mutex> lk(p->mu);
    // the handle and its torj_trace_beam replicas (new replicas inherit it)
    for (size_t k = 0; k < std::max<size_t>(1, p->replicas.size()); k++) {
        torj_plasma_s *q = k == 0 ? p : p->replicas[k];
        q->timing = enable != 0;
        q->ev_used = 0;
        q->timing_calls = 0;
    }
    p->reduce_ms = 0.0;
    p->reduce_calls = 0;
    return 0;
}

int torj_timing_read(torj_plasma_t p, int *calls, double *trace_ms, double *post_ms) {
    if (!p) return fail("bad plasma handle");
    double t = 0.0, q = 0.0;
    for (size_t k = 0; k + 3 <= p->ev_used; k += 3) {
        float a = 0.f, b = 0.f;
        HIPCK(hipEventSynchronize(p->ev_pool[k + 2]));
        HIPCK(hipEventElapsedTime(&a, p->ev_pool[k], p->ev_pool[k + 1]));
        HIPCK(hipEventElapsedTime(&b, p->ev_pool[k + 1], p->ev_pool[k + 2]));
        t += a;
        q += b;
    }
    if (calls) *calls = p->timing_calls;  // a batched call records one triple per batch
    if (trace_ms) *trace_ms = t;
    if (post_ms) *post_ms = q;
    p->ev_used = 0;
    p->timing_calls = 0;
    return 0;
}

int torj_beam_timing_read(torj_plasma_t p, int n_gpus, int *calls, double *trace_ms, double *post_ms,
                          double *reduce_ms) {
    if (!p) return fail("bad plasma handle");
    if (n_gpus < 1) return fail("n_gpus must be >= 1");
    int dev0 = 0;
    HIPCK(hipGetDevice(&dev0));
    // the replica list (torj_timing and beam_replicas take it too): held from the
    // range check on, so a concurrent fan-out cannot change it in between
    std::lock_guard<std::mutex> lk(p->mu);
    if (n_gpus > std::max<int>(1, (int)p->replicas.size()))
        return fail("n_gpus = %d, but the handle has %d replica(s)", n_gpus, std::max<int>(1, (int)p->replicas.size()));
    int rc = 0;
    for (int k = 0; k < n_gpus && rc == 0; k++) {
        torj_plasma_s *q = k == 0 ? p : p->replicas[k];
        if (hipSetDevice(q->device) != hipSuccess)
            rc = fail("hipSetDevice(%d) failed", q->device);
        else if (torj_timing_read(q, calls ? calls + k : nullptr, trace_ms ? trace_ms + k : nullptr,
                                  post_ms ? post_ms + k : nullptr))
            rc = -1;
    }
    (void)hipSetDevice(dev0);  // the caller's device on every path
    if (rc) return rc;
    if (reduce_ms) *reduce_ms = p->reduce_ms;
    p->reduce_ms = 0.0;
    p->reduce_calls = 0;
    return 0;
}

int torj_beam_comm_info(torj_plasma_t p, int n_gpus, int *device, int *nranks, int *rank) {
    if (!p) return fail("bad plasma handle");
    if (n_gpus < 1) return fail("n_gpus must be >= 1");
    if (!device || !nranks || !rank) return fail("device, nranks and rank must be arrays of n_gpus");
    std::lock_guard<std::mutex> lk(p->mu);
    if (n_gpus > std::max<int>(1, (int)p->replicas.size()))
        return fail("n_gpus = %d, but the handle has %d replica(s)", n_gpus, std::max<int>(1, (int)p->replicas.size()));
    // the communicator of the last RCCL reduce (beam_reduce_run keeps one per
    // replica of that fan-out; rebuilt when the replica count changes)
    const bool comm = (int)p->comms.size() == n_gpus;
    for (int k = 0; k < n_gpus; k++) {
        device[k] = (k == 0 ? p : p->replicas[k])->device;
        nranks[k] = 0;
        rank[k] = -1;
        if (comm && p->comms[k]) {
            if (ncclCommCount(p->comms[k], nranks + k) != ncclSuccess ||
                ncclCommUserRank(p->comms[k], rank + k) != ncclSuccess)
                return fail("ncclCommCount / ncclCommUserRank failed for replica %d", k);
        }
    }
    return 0;
}

int torj_set_sched(torj_plasma_t p, int mode, int waves) {
    if (!p) return fail("bad plasma handle");
    if (mode < -1 || mode > 3) return fail("sched mode must be -1, 0, 1, 2 or 3");
    if (waves < 0) return fail("waves must be >= 0");
    p->sched_mode = mode == 2 ? 0 : mode;
    p->lanes_per_ray = mode == 0 ? 1 : (mode == 2 ? 16 : 0);
    p->sched_waves = waves;
    return 0;
}

int torj_trace(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
               const double *N0, const double *weights, int n_psi, const double *grid,
               double *state, int *status, int *steps, double *dP, double *Pdep, double *traj) {
    return torj_trace_ex(p, cfg, n, x0, N0, weights, n_psi, grid, nullptr, nullptr, state, status,
                         steps, dP, Pdep, traj);
}

int torj_trace_ex(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
                  const double *N0, const double *weights, int n_psi, const double *grid,
                  const double *x_launch, const double *s0, double *state, int *status,
                  int *steps, double *dP, double *Pdep, double *traj) {
    if (!p || !cfg) return fail("bad plasma handle or cfg");
    if (n <= 0) return 0;
    // (the grid's host copy is at hand: checked before any device work)
    if (n_psi >= 2 && grid && grid_increasing(n_psi, grid)) return -1;
    RayIO io{};
    io.n = n, io.x0 = x0, io.N0 = N0, io.weights = weights, io.psi_grid = grid, io.x_launch = x_launch, io.s0 = s0;
    io.state = state, io.status = status, io.steps = steps, io.dP_shell = dP, io.P_dep = Pdep, io.traj = traj;
    return trace_staged(p, cfg, io, 1, n_psi, [&](const RayIO &d, int n_psi_d, hipStream_t s) {
        return trace_device(p, cfg, d, n_psi_d, s);
    });
}

int torj_trace_beam(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
                    const double *N0, const double *weights, int n_psi, const double *grid,
                    const double *x_launch, const double *s0, double *state, int *status,
                    int *steps, double *dP, double *Pdep, double *traj, int n_gpus, int n_shards) {
    if (!p || !cfg) return fail("bad plasma handle or cfg");
    if (n < 0 || n_shards < 0) return fail("n and n_shards must be >= 0");
    if (n == 0) {
        if (dP && n_psi > 0) std::fill(dP, dP + n_psi + 1, 0.0);
        return 0;
    }
    if (!x0 || !N0 || !state || !status || !steps) return fail("x0, N0, state, status, steps required");
    const bool depo = n_psi >= 2 && grid;
    if (depo) {
        if (grid_increasing(n_psi, grid)) return -1;
        if (!dP || !Pdep) return fail("deposition needs dP_shell and P_dep");
    }
    const bool same = beam_same_device();
    if (beam_replicas(p, n_gpus, same)) return -1;
    const int S = n_shards > 0 ? std::max(n_shards, n_gpus) : beam_auto_shards(n, n_gpus);
    const bool reduce = depo && (n_gpus > 1 || env_int("TORJ_BEAM_RCCL", 0) != 0);  // read per call (tests toggle it)
    // per-device partial dP_shell, then one all-reduce
    std::vector<double *> d_dP(n_gpus, nullptr);
    RayIO io{};  // the whole beam's host arrays (dP_shell: downloaded here, after the reduce)
    io.n = n, io.x0 = x0, io.N0 = N0, io.weights = weights, io.psi_grid = grid, io.x_launch = x_launch, io.s0 = s0;
    io.state = state, io.status = status, io.steps = steps, io.P_dep = Pdep, io.traj = traj;
    int out = beam_fanout(p, n_gpus, "torj_trace_beam", [&](int k) -> int {
        torj_plasma_s *q = p->replicas[k];
        if (depo) HIPCK(hipMalloc(&d_dP[k], (n_psi + 1) * sizeof(double)));
        return beam_worker(q, cfg, io, S, k, n_gpus, n_psi, d_dP[k]);
    });
    if (!out && reduce) out = beam_reduce(p, n_gpus, d_dP, n_psi, same);
    if (!out && depo) {
        torj_plasma_s *q0 = p->replicas[0];
        if (hipSetDevice(q0->device) != hipSuccess ||
            hipMemcpyAsync(dP, d_dP[0], (n_psi + 1) * sizeof(double), hipMemcpyDeviceToHost,
                           q0->stream) != hipSuccess ||
            hipStreamSynchronize(q0->stream) != hipSuccess)
            out = fail("download of dP_shell failed");
    }
    for (int k = 0; k < n_gpus; k++)
        if (d_dP[k]) {
            (void)hipSetDevice(p->replicas[k]->device);
            (void)hipStreamSynchronize(p->replicas[k]->stream);
            (void)hipFree(d_dP[k]);
        }
    if (!out && !depo) {
        if (dP) std::fill(dP, dP + dP_rows(1, n_psi), 0.0);
        if (Pdep) std::fill(Pdep, Pdep + n, 0.0);
    }
    (void)hipSetDevice(p->device);
    return out;
}

int torj_trace_beam_device(torj_plasma_t p, const torj_trace_cfg *cfg, int n_gpus, int n_psi,
                           const torj_beam_shard *shards) {
    if (!p || !cfg || !shards) return fail("bad plasma handle, cfg or shards");
    const bool same = beam_same_device();
    if (beam_replicas(p, n_gpus, same)) return -1;
    bool depo = n_psi >= 2;
    for (int k = 0; k < n_gpus; k++) {
        if (shards[k].n < 0) return fail("shard %d: n < 0", k);
        depo = depo && shards[k].psi_grid && shards[k].dP_shell;
    }
    if (n_psi >= 2 && !depo) return fail("deposition needs psi_grid and dP_shell on every shard");
    const bool reduce = depo && (n_gpus > 1 || env_int("TORJ_BEAM_RCCL", 0) != 0);
    int out = beam_fanout(p, n_gpus, "torj_trace_beam_device", [&](int k) -> int {
        torj_plasma_s *q = p->replicas[k];
        if (ensure_device(q) || trace_device(q, cfg, shards[k], depo ? n_psi : 0, q->stream)) return -1;
        return torj_trace_check(q, q->stream);  // waits for the stream: queue / grid flags
    });
    if (!out && reduce) {
        std::vector<double *> d_dP(n_gpus);
        for (int k = 0; k < n_gpus; k++) d_dP[k] = shards[k].dP_shell;
        out = beam_reduce(p, n_gpus, d_dP, n_psi, same);
    }
    (void)hipSetDevice(p->device);
    return out;
}

int torj_trace_check(torj_plasma_t p, void *stream) {
    if (!p) return fail("bad plasma handle");
    if (!p->d_flags) return 0;  // no launch yet
    HIPCK(hipSetDevice(p->device));
    HIPCK(hipStreamSynchronize((hipStream_t)stream));
    int flags = 0;  // ORed by every launch on this handle since the last check
    HIPCK(hipMemcpy(&flags, p->d_flags, sizeof(int), hipMemcpyDeviceToHost));
    if (flags) HIPCK(hipMemset(p->d_flags, 0, sizeof(int)));
    if (flags & 1) return fail("psi_dP_dV must be strictly increasing");
    if (flags & 2) return fail("work-queue watchdog fired (ready-queue stalled)");
    if (flags & 4) return fail("work queue did not retire every ray group");
    return 0;
}

}  // extern "C"

