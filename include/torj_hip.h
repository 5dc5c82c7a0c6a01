/*
 * torj_hip.h -- C ABI of libtorj_hip.so, the MI355X-native replacement for the
 * ray-tracing hot path of TorJ.jl (make_ray / make_beam, src/solve.jl).
 *
 * The reference has no FFI: everything is Julia.  Each entry point below names
 * the Julia function whose behaviour it replaces (file:line in the TorJ.jl
 * repository); INTEGRATION.md shows the `ccall` bindings a TorJ maintainer
 * would add (torj.jl_amd/julia/TorJHIP.jl) and the Python ctypes mirror used by
 * this repository's tests (torj.jl_amd/torj_hip).
 *
 * Conventions
 *  - Plain C types only.  Return value: 0 = success, <0 = error; the message of
 *    the last error on the calling thread is returned by torj_last_error().
 *    No exception or longjmp ever crosses this boundary.
 *  - Per-ray 3-vectors are COMPONENT-MAJOR ("SoA"): v[c*n + i] is component c of
 *    ray i.  This is exactly the memory of a Julia `n x 3` Matrix{Float64}
 *    (column-major), e.g. the ray_positions returned by launch_peripheral_rays
 *    (src/launch.jl:84-86), so Julia passes them without copying.
 *  - 2-D maps are (nR x nZ) column-major (R fastest), i.e. Julia matrices.
 *  - Functions without the _device suffix take HOST pointers owned by the
 *    caller and valid only for the call (Julia: GC.@preserve); they copy to the
 *    GPU, run, copy back and synchronise.  *_device functions take device
 *    pointers and a hipStream_t (as void*), enqueue and return immediately.
 *  - All arithmetic is fp64.
 *  - Every compute entry point runs on the GPU (HIP, gfx950).  There is no
 *    CPU fallback: without a usable GPU they return an error.
 */
#ifndef TORJ_HIP_H
#define TORJ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TORJ_ABI_VERSION 8  /* 3: torj_trace_beam, sticky launch flags; 4: 8 work counters;
                               5: torj_trace_beam_device, torj_power_deposition_profile;
                               6: torj_beam_timing_read, torj_trace_beam's automatic shards;
                               7: torj_build_id; 8: torj_beam_comm_info; still 8 (symbols added,
                               nothing changed): torj_trace_beams, torj_trace_beams_device,
                               torj_ray_entry_beams_gpu, torj_ray_entry_beams_device;
                               still 8 (four more symbols, nothing changed):
                               torj_trace_beams_plasmas, torj_trace_beams_plasmas_device,
                               torj_ray_entry_beams_plasmas_gpu, torj_ray_entry_beams_plasmas_device;
                               still 8 (four more symbols, nothing changed): torj_plasma_update,
                               torj_plasma_update_from_coefs, torj_plasma_update_profiles,
                               torj_plasma_get_cell_table;
                               still 8 (three more symbols, nothing changed): torj_plasma_update_gpu,
                               torj_plasma_update_profiles_gpu, torj_plasma_update_device;
                               still 8 (one more symbol, nothing changed): torj_make_beams;
                               still 8 (two more symbols, nothing changed): torj_ray_profile,
                               torj_ray_profile_device */

/* per-ray status codes (replace the reference's @assert / unhandled returns) */
enum torj_status {
    TORJ_RAY_OK = 0,          /* ran all steps */
    TORJ_RAY_LEFT_PLASMA = 1, /* psi > psi_exit at a chunk boundary (src/solve.jl:174) */
    TORJ_RAY_ABSORBED = 2,    /* P < P_min at a chunk boundary (src/solve.jl:176) */
    TORJ_RAY_NAN = 3,         /* non-finite state (e.g. upper-hybrid resonance) */
    TORJ_RAY_REFLECTED = 4,   /* N_s^2 <= 0 at the plasma edge (src/solve.jl:57-59) */
    TORJ_RAY_ENTRY_FAIL = 5,  /* first_point / refraction assertions (src/solve.jl:32,138,141) */
    TORJ_RAY_MAX_STEPS = 6    /* integrator 1: accepted-step capacity n_steps exhausted */
};

typedef struct torj_plasma_s *torj_plasma_t;

/* ---- library / device ---------------------------------------------------- */
int torj_abi_version(void);
/* identity of this build: 16 hex digits of a hash over the library's sources
 * and compile flags (csrc/Makefile).  Profiles record it, and bench.py uses a
 * committed profile only when its build id equals the loaded library's. */
const char *torj_build_id(void);
const char *torj_last_error(void);
int torj_device_count(int *n);

/* abs_Al_init(N_absz) (src/absorption.jl:1-7): Gauss-Legendre order of the
 * Albajar resonance-ellipse integral (process-global, like the reference's
 * module globals _int_absz/_int_weights, src/constants.jl:7-8).  1 <= n <= 64.
 * Absorption calls fail with the reference's ErrorException message
 * (src/absorption.jl:173-175) until this has been called.  Also reads
 * TORJ_TINY_ALPHA (m^-1, default 1e-20; 0 = off): fixed-step ray tracing skips
 * a harmonic integral whose rigorous bound on its share of alpha is below it
 * (tau moves by < 2 TORJ_TINY_ALPHA per metre of ray). */
int torj_abs_al_init(int n);

/* ---- Plasma (src/plasma.jl:2-58) ----------------------------------------- */
/* Plasma(R_coords, Z_coords, psi_norm_data, psi_prof, ne_prof, Te_prof, Br_data,
 *        Bz_data, Bϕ_data, eqt1d_psi_norm, eqt1d_volume)   (src/plasma.jl:30-58)
 * Builds the Interpolations.jl-equivalent cubic B-spline coefficients (Line()
 * boundary/extrapolation) on the host and uploads them to `device`. */
int torj_plasma_create(int nR, int nZ, const double *R_coords, const double *Z_coords,
                       const double *psi_norm_data, int n_prof, const double *psi_prof,
                       const double *ne_prof, const double *Te_prof, const double *Br_data,
                       const double *Bz_data, const double *Bphi_data, int n_eq,
                       const double *eqt1d_psi_norm, const double *eqt1d_volume, int device,
                       torj_plasma_t *out);
/* Same, from B-spline coefficient arrays already built by Interpolations.jl
 * (parent(spl.itp.itp.coefs): (nR+2) x (nZ+2) column-major each; field order
 * psi, ln ne, ln Te, Br, Bz, Bphi) and the 1-D volume spline coefficients
 * (n_vol+2 over the uniform psi range [vol_psi1, vol_psin]). */
int torj_plasma_create_from_coefs(int nR, int nZ, double R1, double Rn, double Z1, double Zn,
                                  const double *coef_psi, const double *coef_lnne,
                                  const double *coef_lnTe, const double *coef_Br,
                                  const double *coef_Bz, const double *coef_Bphi, int n_vol,
                                  double vol_psi1, double vol_psin, const double *vol_coefs,
                                  double psi_prof_max, int device, torj_plasma_t *out);
int torj_plasma_destroy(torj_plasma_t p);
/* field: 0 psi, 1 ln ne, 2 ln Te, 3 Br, 4 Bz, 5 Bphi.  out: (nR+2)*(nZ+2), column-major */
int torj_plasma_get_coefs(torj_plasma_t p, int field, double *out);
double torj_plasma_psi_prof_max(torj_plasma_t p);
/* plasma.volume_psi_spline at n points (host) */
int torj_plasma_volume(torj_plasma_t p, int n, const double *psi, double *vol);

/* ---- a live handle's physics replaced in place ------------------------------
 * A transport loop or a pool of time slices keeps its handles: their workspaces,
 * streams, events, replicas and communicators, scheduling and timing settings all
 * stay, and only the equilibrium and the kinetic profiles change.  The grid SIZE
 * (nR, nZ) is the handle's; the box (the ends of R_coords / Z_coords, or R1 .. Zn),
 * psi_prof_max and the volume spline follow the new arguments.
 *
 * The host arrays are consumed before the call returns, and the new host state is
 * built by the functions torj_plasma_create[_from_coefs] use, so
 * torj_plasma_get_coefs and every host entry give bit for bit what a fresh handle
 * gives.  Every argument is checked, and the new state is complete, before the
 * handle is touched: a refused call (NULL handle or pointer, n_prof < 2, n_eq < 2,
 * n_vol < 2; the message names the argument) leaves the handle as it was.
 *
 * Before the handle's first GPU use the update is host-only.  Afterwards the new
 * coefficients are copied to the device and the per-cell power table of the split
 * pipeline's trajectory kernels is rebuilt from them there (k_cell_table), both
 * enqueued on `stream` without any synchronisation: traces enqueued earlier on the
 * stream finish on the old plasma, traces enqueued later see the new one.  `stream`
 * is the handle's one stream (as torj_trace_device_ex: one stream per handle at a
 * time; NULL is the legacy default stream, joined the same way); the handle's own
 * stream, on which the host-pointer entries run, waits for the update on the
 * device.  Replicas made by torj_trace_beam[_device] get the same update, each on
 * its own device and stream.  A handle that another handle's
 * torj_trace_beams_plasmas_device launch lists falls under that call's lifetime
 * rule: updating it before that launch has been checked (torj_trace_check) is a
 * caller error.
 *
 * Rounding: a handle's first GPU use builds the cell table on the host in long
 * double; an update rebuilds it on the device in double-double arithmetic (each
 * entry rounded once from >= 100 bits, the more accurate of the two).  Only the
 * split pipeline reads the table, so split-pipeline traces of an updated handle
 * agree with a fresh handle's to rounding (~1e-15 in x and N), and every other
 * result (one-shot, work-queue, adaptive and multi-beam traces, ray entry, point
 * evaluations) is bit-identical. */
/* the arguments of torj_plasma_create without nR, nZ, device, out */
int torj_plasma_update(torj_plasma_t p, const double *R_coords, const double *Z_coords,
                       const double *psi_norm_data, int n_prof, const double *psi_prof,
                       const double *ne_prof, const double *Te_prof, const double *Br_data,
                       const double *Bz_data, const double *Bphi_data, int n_eq,
                       const double *eqt1d_psi_norm, const double *eqt1d_volume, void *stream);
/* the arguments of torj_plasma_create_from_coefs without nR, nZ, device, out.  The
 * handle keeps no node data afterwards: torj_plasma_update_profiles is refused. */
int torj_plasma_update_from_coefs(torj_plasma_t p, double R1, double Rn, double Z1, double Zn,
                                  const double *coef_psi, const double *coef_lnne,
                                  const double *coef_lnTe, const double *coef_Br,
                                  const double *coef_Bz, const double *coef_Bphi, int n_vol,
                                  double vol_psi1, double vol_psin, const double *vol_coefs,
                                  double psi_prof_max, void *stream);
/* new kinetic profiles on the handle's equilibrium: make_2d_prof_spline
 * (src/plasma.jl:16-22) on the psi_norm_data that torj_plasma_create or
 * torj_plasma_update last gave (the handle keeps a host copy).  Only the ln ne and
 * ln Te coefficients and psi_prof_max change.  Refused on a handle whose
 * equilibrium came as coefficients. */
int torj_plasma_update_profiles(torj_plasma_t p, int n_prof, const double *psi_prof,
                                const double *ne_prof, const double *Te_prof, void *stream);
/* ---- ... with the 2-D spline coefficients built on the device ------------------
 * The three calls below do what torj_plasma_update and torj_plasma_update_profiles
 * do, but the six (or two) 2-D B-spline prefilters, the host's ~2 ms per plasma at
 * 129 x 129 nodes, run on the GPU in `stream`'s order, ahead of k_cell_table:
 * make_2d_prof_spline's node map, a prefilter along R and one along Z, the host's
 * operation sequences under IEEE arithmetic, so the device coefficients are bit for
 * bit the host's.  The host keeps the 1-D parts (the profiles' resampling, log and
 * 1-D prefilter, the volume spline, psi_prof_max, the box) with the functions the
 * host updates use.
 *
 * Checks and refusals are torj_plasma_update's (the message starts with the
 * function's name and names the argument); further refusals, which also leave the
 * handle as it was: no usable GPU for the handle's device, and a profiles-only call
 * on a handle whose equilibrium came as coefficients.  A handle never used on the
 * GPU gets its device state first.  Host arrays are consumed before the call
 * returns (copied in stream order into a grow-only staging buffer of the handle:
 * 0.53 MB for a full update at 129 x 129, about 1 KB for a profiles-only one);
 * nothing synchronises.  The stream rules are torj_plasma_update's.  The handle
 * keeps the psi node map on the device for later profiles-only calls (a handle
 * that only has the host copy uploads it on first need).  Replicas get the built
 * coefficients by a device copy (a peer copy across devices) behind the build,
 * then rebuild their own cell tables.
 *
 * HOST READS SYNCHRONISE.  After one of these calls the handle's host copy of the
 * coefficients (and, after torj_plasma_update_device, of psi_norm_data) is stale.
 * The host readers -- torj_plasma_get_coefs, the host torj_ray_entry, the host
 * torj_plasma_update_profiles, and the creation of replicas by torj_trace_beam --
 * first wait for the build's event and download the copy, once; a later host
 * update (torj_plasma_update, torj_plasma_update_from_coefs) replaces it without a
 * download.  The GPU entries (torj_ray_entry_gpu, the traces, torj_eval_plasma)
 * never read the host copy. */
/* torj_plasma_update's arguments; all arrays are host arrays */
int torj_plasma_update_gpu(torj_plasma_t p, const double *R_coords, const double *Z_coords,
                           const double *psi_norm_data, int n_prof, const double *psi_prof,
                           const double *ne_prof, const double *Te_prof, const double *Br_data,
                           const double *Bz_data, const double *Bphi_data, int n_eq,
                           const double *eqt1d_psi_norm, const double *eqt1d_volume, void *stream);
/* torj_plasma_update_profiles' arguments */
int torj_plasma_update_profiles_gpu(torj_plasma_t p, int n_prof, const double *psi_prof,
                                    const double *ne_prof, const double *Te_prof, void *stream);
/* torj_plasma_update_gpu with psi_norm_data, Br_data, Bz_data, Bphi_data (nR x nZ,
 * R fastest) as device pointers on the handle's device, read in `stream`'s order:
 * they must stay valid and unchanged until the stream has passed the call.
 * R_coords, Z_coords, the profiles and the volume table stay host arrays. */
int torj_plasma_update_device(torj_plasma_t p, const double *R_coords, const double *Z_coords,
                              const double *psi_norm_data, int n_prof, const double *psi_prof,
                              const double *ne_prof, const double *Te_prof, const double *Br_data,
                              const double *Bz_data, const double *Bphi_data, int n_eq,
                              const double *eqt1d_psi_norm, const double *eqt1d_volume, void *stream);
/* the per-cell power table as it stands on the device: (nR-1) x (nZ-1) cells, R
 * fastest, 96 doubles each (field slot f of Br, Bphi, Bz, ln ne, ln Te, psi at
 * f * 16, the coefficient of sZ^j sR^i at j * 4 + i, per metre).  Waits for the
 * handle's stream.  An error before the handle's first GPU use. */
int torj_plasma_get_cell_table(torj_plasma_t p, double *out);

/* ---- point evaluations (GPU; mirror the reference's unit-tested functions) -- */
/* Per point i (x, N component-major 3 x n), out is 13 x n component-major:
 *   0-2  B_spline(plasma, x)            (src/plasma.jl:73-81)
 *   3    n_e(plasma, x)                 (src/plasma.jl:83-85)
 *   4    T_e(plasma, x)                 (src/plasma.jl:87-89)
 *   5    evaluate(psi_norm_spline, x)   (src/plasma.jl:61-65)
 *   6-8  X, Y, N_par of eval_plasma     (src/dispersion.jl:7-15)
 *   9-11 b of eval_plasma
 *   12   |B|                                                             */
int torj_eval_plasma(torj_plasma_t p, int n, const double *x, const double *N, double omega,
                     double *out);
/* dispersion_relation (src/dispersion.jl:34-39), the normalised Hamiltonian
 * RHS of gradΛ! (src/solve.jl:85-93; du = dx/ds, dN/ds, 6 x n) and α_approx
 * (src/absorption.jl:228-235; pass alpha = NULL to skip). */
int torj_dispersion(torj_plasma_t p, int n, const double *x, const double *N, double omega,
                    int mode, double *D, double *du, double *alpha);
/* abs_Albajar_fast(omega, X, Y, N_abs, N_par, Te, mode) (src/absorption.jl:191-226),
 * batched over n tuples (arrays of length n). */
int torj_abs_albajar_fast(int n, const double *omega, const double *X, const double *Y,
                          const double *N_abs, const double *N_par, const double *Te, int mode,
                          double *alpha);
/* refractive_index_sq(X, Y, N_par, mode) (src/dispersion.jl:29-32), batched */
/* Warm-plasma absorption alpha (src/general_absorption.jl:1328-1337, repaired
 * as described in DESIGN.md): warmdisp's N_perp^2 with the weakly (iwarm 1) or
 * fully (iwarm 3) relativistic dielectric tensor, lrm = min(5, larmornumber),
 * alpha = 2 Im(N_perp^2) omega/c / |dD/dN| (inv_dDdN = 1/|dD/dN|); Nperp2 (may
 * be NULL) receives N_perp^2 as (re, im) pairs.  GPU, batched (host arrays). */
int torj_alpha_warm(int n, const double *omega, const double *X, const double *Y,
                    const double *N_abs, const double *N_par, const double *Te,
                    const double *inv_dDdN, int mode, int iwarm, double *alpha, double *Nperp2);

int torj_refractive_index_sq(int n, const double *X, const double *Y, const double *N_par,
                             int mode, double *out);

/* ---- launch (host) ------------------------------------------------------- */
/* IMAS.pol_tor_angles_2_vector(pol, tor) as called at src/solve.jl:211 */
void torj_pol_tor_angles_2_vector(double pol, double tor, double N[3]);
/* launch_peripheral_rays (src/launch.jl:24-132).  Call with pos == NULL to get
 * the ray count in *n_rays; then with arrays of that size (pos, dir
 * component-major 3 x n).  Returns -1 (ArgumentError) for N_rings < 2. */
int torj_launch_peripheral_rays(const double x0[3], const double N0[3], double w,
                                double inverse_curvature_radius, double f, int N_rings,
                                int min_azimuthal_points, int normalize_weight_sum, int *n_rays,
                                double *pos, double *dir, double *weights);

/* ---- ray entry: first_point + vacuum_plasma_refraction (src/solve.jl:7-74) --
 * x0, N0: vacuum launch points/directions (3 x n); outputs the in-plasma start
 * point, refracted N, vacuum path length s0 and a status per ray. */
int torj_ray_entry(torj_plasma_t p, int n, const double *x0, const double *N0, double omega,
                   int mode, double *x_plasma, double *N_plasma, double *s0, int *status);
/* Same computation on the GPU (one lane per ray), device pointers, async on
 * `stream` (hipStream_t or NULL).  Replaces the per-ray host bisection + NLsolve
 * of make_beam's ray loop (src/solve.jl:219-221 -> :137-141). */
int torj_ray_entry_device(torj_plasma_t p, int n, const double *x0, const double *N0,
                          double omega, int mode, double *x_plasma, double *N_plasma, double *s0,
                          int *status, void *stream);
/* Host pointers, GPU compute (upload, torj_ray_entry_device, download). */
int torj_ray_entry_gpu(torj_plasma_t p, int n, const double *x0, const double *N0, double omega,
                       int mode, double *x_plasma, double *N_plasma, double *s0, int *status);

/* ---- the hot path: ray stepping (src/solve.jl:144-177) ------------------- */
typedef struct {
    double omega;     /* 2 pi f */
    int mode;         /* +1 X-mode, -1 O-mode (src/solve.jl:110) */
    double ds;        /* fixed RK4 step [m]; the reference caps dtmax at 1e-4 (src/solve.jl:157) */
    int n_steps;      /* steps per ray (s_max / ds) */
    int chunk_steps;  /* termination checks every chunk_steps (reference: 100 chunks, src/solve.jl:145) */
    double psi_exit;  /* 1.0 in the reference (src/solve.jl:174) */
    double P_min;     /* 1e-6 in the reference (src/solve.jl:176) */
    int absorption;   /* optical depth model: 0 none; 1 abs_Albajar_fast (src/absorption.jl:191-226);
                         2 warm weakly relativistic, 3 warm fully relativistic (the repaired
                         src/general_absorption.jl alpha, :1328-1337; 3 is what it hard-codes,
                         2 is BASELINE's C5) -- see torj_alpha_warm */
    int traj_stride;  /* 0: no trajectory; else save (x,y,z,tau) every traj_stride steps */
    int deposition;   /* 0: in-kernel psi-shell binning of the RK4 steps (fast, default);
                         1: the reference's power_deposition_profile (src/plasma.jl:91-151):
                            not-a-knot cubic splines of psi(s) and dP/ds = P alpha through
                            make_ray's saved points, boundary roots paired per shell,
                            |integral| per pair, outside-in walk -- needs torj_trace_ex */
    int integrator;   /* 0: fixed-step classic RK4 of n_steps steps of ds (default);
                         1: adaptive, as the reference's solve() (src/solve.jl:144-162):
                            Tsit5 5(4) on u = (x, N, P) with DiffEq's PI step control and
                            initial-step heuristic, abstol/reltol below, dtmax = ds, over
                            n_chunks tspans of s_max/n_chunks starting at s0 (each chunk
                            restarts the integrator); n_steps is then the per-ray capacity
                            of accepted steps (status MAX_STEPS when exceeded) */
    double abstol, reltol;  /* integrator 1: 1e-6, 1e-6 in the reference (src/solve.jl:157) */
    double s_max;     /* integrator 1: path length in the plasma (make_ray's s_max) */
    int n_chunks;     /* integrator 1: 100 in the reference (src/solve.jl:145) */
} torj_trace_cfg;

/* Host-pointer form.  x0, N0: in-plasma start states (3 x n); weights (n, may
 * be NULL = all 1); psi_grid (n_psi, may be n_psi = 0: no deposition).
 * Outputs: state 7 x n (x, y, z, Nx, Ny, Nz, tau with P = exp(-tau)),
 * status n, steps n; dP_shell n_psi + 1: [j] = sum_rays w * (power deposited
 * in psi shell [psi_grid[j], psi_grid[j+1]]) for j < n_psi-1, [n_psi-1] = 0,
 * [n_psi] = sum_rays w * P_dep(ray); P_dep n (per ray, unweighted).  traj:
 * (n_steps/traj_stride) x 5 x n = (x, y, z, tau, s) every traj_stride (accepted)
 * steps, s the arc length from the vacuum launch point; NaN after a ray stops.  Any output may be
 * NULL.  Divide dP_shell[j] by the shell volume to get make_beam's dP_dV
 * (src/plasma.jl:141, src/solve.jl:237-240). */
int torj_trace(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
               const double *N0, const double *weights, int n_psi, const double *psi_grid,
               double *state, int *status, int *steps, double *dP_shell, double *P_dep,
               double *traj);

/* With the vacuum launch points x_launch (3 x n, make_ray's first point, s = 0)
 * and path lengths s0 (n) to the entry point -- what cfg->deposition = 1 needs
 * to rebuild make_ray's s / psi vectors.  With deposition = 1, dP_shell[j] is
 * sum_rays w dP_j of the reference profile, dP_shell[n_psi] = sum_rays w P and
 * P_dep[i] = the ray's deposited power P (src/plasma.jl:140-147). */
int torj_trace_ex(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
                  const double *N0, const double *weights, int n_psi, const double *psi_grid,
                  const double *x_launch, const double *s0, double *state, int *status,
                  int *steps, double *dP_shell, double *P_dep, double *traj);

/* Device-pointer form (inputs resident in HBM; what bench.py times).
 * dP_shell (n_psi+1) is ACCUMULATED into (zero it first).  counters (may be
 * NULL): 8 x uint64 accumulated, the basis of the algorithmic FLOP count
 * (torj_hip/flops.py): [0] ray-steps, [1] RHS evaluations, then
 *   absorption 1 (Albajar): [2] calls reaching the harmonic sum, [3] harmonic
 *     integrals evaluated, [4] Bessel-series terms, [5] harmonic integrals found
 *     exactly zero without their node loop, [6] harmonic integrals skipped as
 *     provably below an ulp of the sum (alpha bit-identical), [7] harmonic
 *     integrals found exactly zero in calls settled before the polarisation
 *     vector (every harmonic present an exact zero: alpha = 0, no call
 *     reaches the harmonic sum);
 *   absorption 2 (warm, iwarm 1): [2] Faddeeva evaluations by the asymptotic
 *     series (|z| >= 16, of [3]), [3] Faddeeva evaluations, [4] warmdisp
 *     passes, [5] passes x Larmor order lrm,
 *     [6] sum lrm, [7] sum lrm^2 (one warm alpha per RHS evaluation);
 *   absorption 0 / 3: [2..7] 0.
 * stream: hipStream_t or NULL. */
int torj_trace_device(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
                      const double *N0, const double *weights, int n_psi,
                      const double *psi_grid, double *state, int *status, int *steps,
                      double *dP_shell, double *P_dep, double *traj, uint64_t *counters,
                      void *stream);
int torj_trace_device_ex(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
                         const double *N0, const double *weights, int n_psi,
                         const double *psi_grid, const double *x_launch, const double *s0,
                         double *state, int *status, int *steps, double *dP_shell, double *P_dep,
                         double *traj, uint64_t *counters, void *stream);

/* ---- many small beams of differing frequency and mode in one launch -------
 * (no reference counterpart: an EC system of tens of launchers is tens of
 * make_beam calls there, src/solve.jl:209-242).  The rays of n_beams beams are
 * concatenated: beam b owns rays beam_off[b] .. beam_off[b+1] - 1 of every
 * per-ray array (beam_off[0] = 0, non-decreasing, empty beams allowed; the
 * arrays hold n = beam_off[n_beams] rays), is traced with omega[b] and mode[b]
 * (cfg->omega and cfg->mode are ignored; every other cfg field is shared) and
 * deposits into row b of dP_shell, n_beams rows of n_psi + 1 laid out as
 * torj_trace's one.  n_beams <= 4096.  One launch of the one-shot kernel whatever
 * the size (torj_set_sched modes 1 and 3 are refused), with absorption 0 or 1
 * and integrator 0 only.  Lanes per ray as for a single beam (16 for Albajar
 * without binned deposition while the launch's waves fit two per SIMD;
 * torj_set_sched 0 / 2 and env TORJ_LPR=1 force it).  No wave of the launch
 * mixes beams and a beam's waves hold the rays they would hold were the beam
 * traced alone, so every per-ray output, and with deposition = 1 every dP_shell
 * row, equals bit for bit what torj_trace_device_ex gives for that beam with
 * the same lanes per ray (binned rows: up to the order of the atomic sums).
 * With deposition = 1 the workspace holds all n rays at once: a launch beyond
 * the budget (TORJ_WS_GB) is an error, not batched -- trace such beams in
 * separate calls.
 * beam_off, omega and mode are HOST arrays in both forms (n_beams + 1, n_beams,
 * n_beams) and are consumed before the call returns: the caller may overwrite
 * them at once, also between two calls enqueued on one stream.
 * _device: every other pointer is device memory, enqueued on `stream` as
 * torj_trace_device_ex is (NULL stream, torj_timing, torj_trace_check's sticky
 * flags, one stream per handle); dP_shell is accumulated into; counters are sums
 * over all beams.  torj_trace_beams: host pointers, synchronous, checked. */
int torj_trace_beams_device(torj_plasma_t p, const torj_trace_cfg *cfg, int n_beams,
                            const int *beam_off, const double *omega, const int *mode,
                            const double *x0, const double *N0, const double *weights, int n_psi,
                            const double *psi_grid, const double *x_launch, const double *s0,
                            double *state, int *status, int *steps, double *dP_shell,
                            double *P_dep, double *traj, uint64_t *counters, void *stream);
int torj_trace_beams(torj_plasma_t p, const torj_trace_cfg *cfg, int n_beams, const int *beam_off,
                     const double *omega, const int *mode, const double *x0, const double *N0,
                     const double *weights, int n_psi, const double *psi_grid,
                     const double *x_launch, const double *s0, double *state, int *status,
                     int *steps, double *dP_shell, double *P_dep, double *traj);
/* torj_ray_entry_device / _gpu for the same concatenated beams: ray i enters
 * with its beam's omega and mode (host tables as above). */
int torj_ray_entry_beams_device(torj_plasma_t p, int n_beams, const int *beam_off,
                                const double *omega, const int *mode, const double *x0,
                                const double *N0, double *x_plasma, double *N_plasma, double *s0,
                                int *status, void *stream);
int torj_ray_entry_beams_gpu(torj_plasma_t p, int n_beams, const int *beam_off,
                             const double *omega, const int *mode, const double *x0,
                             const double *N0, double *x_plasma, double *N_plasma, double *s0,
                             int *status);

/* ---- many small beams through differing plasmas in one launch -------------
 * The multi-beam calls above with a plasma per beam: every time slice of a
 * pulse, a density or temperature scan, an ensemble of perturbed equilibria,
 * each a handful of small beams, share one launch instead of one launch per
 * plasma.  Beam b is traced through plasmas[beam_plasma[b]], 0 <= beam_plasma[b]
 * < n_plasmas <= 4096; a plasma may be listed twice or used by no beam, and the
 * plasmas' grids (nR, nZ, ranges) may differ.  The ray entry uses each plasma's
 * own psi_prof_max.  cfg, psi_exit included, and psi_grid are shared.
 * p is the launch's handle as in every other call: it gives the stream of a
 * NULL `stream`, the scratch buffers and the workspace budget, the sticky flags
 * torj_trace_check(p, ...) reads, torj_timing and the torj_set_sched knobs
 * (lanes per ray are chosen on the whole launch, as above).  p may be listed or
 * not; its own plasma is used only by beams that name it.  Every listed handle
 * must be on p's device (another device is refused, not supported).
 * plasmas and beam_plasma are HOST arrays in both forms (n_plasmas, n_beams),
 * consumed before the call returns like beam_off, omega and mode.
 * Lifetime: the enqueued kernels read the listed handles' device coefficients.
 * Destroying a listed handle before torj_trace_check(p, stream) (or a
 * synchronisation of the stream) has returned is a caller error, the same rule
 * as for every device pointer of the call.  A listed handle never used on the
 * GPU before gets its device state here (allocations and a synchronous upload
 * of its coefficients, once).
 * Results: every per-ray output, and with deposition = 1 row b of dP_shell,
 * equals bit for bit what torj_trace_device_ex gives for beam b alone on
 * plasmas[beam_plasma[b]] with the same lanes per ray; with n_plasmas = 1 the
 * call is torj_trace_beams_device on that plasma.  Restrictions as above:
 * absorption 0 / 1, integrator 0, torj_set_sched -1 / 0 / 2, no ray batches. */
int torj_trace_beams_plasmas_device(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                                    const int *beam_plasma, const torj_trace_cfg *cfg, int n_beams,
                                    const int *beam_off, const double *omega, const int *mode,
                                    const double *x0, const double *N0, const double *weights,
                                    int n_psi, const double *psi_grid, const double *x_launch,
                                    const double *s0, double *state, int *status, int *steps,
                                    double *dP_shell, double *P_dep, double *traj,
                                    uint64_t *counters, void *stream);
int torj_trace_beams_plasmas(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                             const int *beam_plasma, const torj_trace_cfg *cfg, int n_beams,
                             const int *beam_off, const double *omega, const int *mode,
                             const double *x0, const double *N0, const double *weights, int n_psi,
                             const double *psi_grid, const double *x_launch, const double *s0,
                             double *state, int *status, int *steps, double *dP_shell,
                             double *P_dep, double *traj);
int torj_ray_entry_beams_plasmas_device(torj_plasma_t p, int n_plasmas,
                                        const torj_plasma_t *plasmas, const int *beam_plasma,
                                        int n_beams, const int *beam_off, const double *omega,
                                        const int *mode, const double *x0, const double *N0,
                                        double *x_plasma, double *N_plasma, double *s0,
                                        int *status, void *stream);
int torj_ray_entry_beams_plasmas_gpu(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                                     const int *beam_plasma, int n_beams, const int *beam_off,
                                     const double *omega, const int *mode, const double *x0,
                                     const double *N0, double *x_plasma, double *N_plasma,
                                     double *s0, int *status);

/* ---- ray profiles: N, the plasma parameters and alpha at every saved point of a ray ----
 * What the reference computes along a ray and its validation reads point by point
 * (test/tests/test_trajectory.jl, test_absorption.jl): the rays of n_beams small
 * beams are traced as torj_trace_beams[_plasmas] traces them without deposition, and
 * per saved point one row of TORJ_PROF_NCOL columns is written, each column the named
 * reference function at the row's (x, N) with the beam's omega and mode and the
 * beam's plasma.
 * Beams: beam_off, omega, mode (HOST tables, consumed before the call returns) as in
 * torj_trace_beams, empty beams allowed, a single beam is n_beams = 1.  n_plasmas == 0
 * and plasmas == NULL send every beam through p (as torj_make_beams); else beam b goes
 * through plasmas[beam_plasma[b]] under torj_trace_beams_plasmas' rules.
 * cfg is read as torj_trace_beams reads it (ds, n_steps, chunk_steps, psi_exit, P_min,
 * absorption, traj_stride, integrator; omega and mode are the beams'); deposition is
 * not read.  s0 (n, the arc length at the entry point) may be NULL: s then counts from
 * the entry point.  Restrictions are torj_trace_beams': absorption 0 / 1, integrator 0,
 * torj_set_sched -1 / 0 / 2; lanes per ray are chosen as there.
 * prof: n_rows x TORJ_PROF_NCOL x n doubles, n = beam_off[n_beams], rows slowest, a
 * column contiguous over the rays (traj's layout): prof[(k * TORJ_PROF_NCOL + c) * n + i].
 * n_rows must equal n_steps / traj_stride + 1.  Row 0 is the entry point (step 0), row k
 * step k * traj_stride, so traj's sample k - 1 is row k.  Row k of ray i is written iff
 * k * traj_stride <= steps[i]; every other row of that ray is NaN in all columns.
 * state, status, steps: torj_trace_beams' outputs, each may be NULL.  With the same
 * lanes per ray they, and columns 0-2, 6, 7 against traj, are what torj_trace_beams
 * gives bit for bit (the trace kernel is k_trace_beams' code).  Columns ALPHA and DP_DS
 * are torj_dispersion's alpha at the row's (x, N): abs_Albajar_fast chooses per wave of
 * 64 rays of a row, so between launches of differing rays they agree to the alpha bar
 * (1e-10 relative), not to the bit; every other column does not depend on the other rays.
 * Refusals come before any device work: torj_trace_beams' by their texts; the call's
 * own start with "torj_ray_profile:" and name the argument (prof NULL, traj_stride < 1,
 * n_steps < 1, n_rows with the expected value).
 * A warm alpha along the cold-traced ray is one further call: columns X_PL, Y_PL, N_ABS,
 * N_PAR, TE (18, 19, 21, 20, 13) and the reciprocal of column DLAMBDA_DN (24) are
 * torj_alpha_warm's inputs
 * X, Y, N_abs, N_par, Te, inv_dDdN.
 * _device: every pointer but the host tables is device memory; enqueued on `stream`
 * as torj_trace_beams_device is (NULL stream, torj_timing: the trace, then the point
 * kernel; one stream per handle: the tables go through the handle's scratch; check
 * with torj_trace_check).  torj_ray_profile: host pointers, synchronous, checked; it
 * allocates the table on the device for the call (failure is an error naming the
 * byte count). */
enum {
    TORJ_PROF_X = 0, TORJ_PROF_Y, TORJ_PROF_Z, /* 0-2: the point x, y, z [m] */
    TORJ_PROF_NX, TORJ_PROF_NY, TORJ_PROF_NZ,      /* 3-5: the refractive index vector N */
    TORJ_PROF_TAU,      /* 6: optical depth */
    TORJ_PROF_S,        /* 7: arc length as traj stores it, s0 + step * ds */
    TORJ_PROF_P,        /* 8: P = exp(-tau) */
    TORJ_PROF_ALPHA,    /* 9: alpha_approx(x, N) (src/absorption.jl:228-235); 0 for absorption = 0 */
    TORJ_PROF_DP_DS,    /* 10: dP/ds = P alpha (src/solve.jl:171), also in row 0: make_ray's leading 0
                           there (src/solve.jl:151) is its padding, not alpha, and is not imitated */
    TORJ_PROF_PSI,      /* 11: evaluate(psi_norm_spline, x) */
    TORJ_PROF_NE, TORJ_PROF_TE,                    /* 12, 13: n_e [m^-3], T_e [eV] */
    TORJ_PROF_BX, TORJ_PROF_BY, TORJ_PROF_BZ,      /* 14-16: B_spline [T] */
    TORJ_PROF_B_ABS,    /* 17: |B| */
    TORJ_PROF_X_PL, TORJ_PROF_Y_PL, TORJ_PROF_N_PAR, /* 18-20: X, Y, N_par of eval_plasma */
    TORJ_PROF_N_ABS,    /* 21: |N| */
    TORJ_PROF_NS2,      /* 22: refractive_index_sq(X, Y, N_par, mode): the cold index the ray should sit on */
    TORJ_PROF_LAMBDA,   /* 23: dispersion_relation(x, N): the integrator's drift off Lambda = 0 */
    TORJ_PROF_DLAMBDA_DN, /* 24: |dLambda/dN|, gradLambda!'s normalisation (src/solve.jl:91) */
    TORJ_PROF_NCOL      /* 25 */
};
int torj_ray_profile_device(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                            const int *beam_plasma, const torj_trace_cfg *cfg, int n_beams,
                            const int *beam_off, const double *omega, const int *mode,
                            const double *x0, const double *N0, const double *s0, int n_rows,
                            double *prof, double *state, int *status, int *steps, void *stream);
int torj_ray_profile(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                     const int *beam_plasma, const torj_trace_cfg *cfg, int n_beams,
                     const int *beam_off, const double *omega, const int *mode, const double *x0,
                     const double *N0, const double *s0, int n_rows, double *prof, double *state,
                     int *status, int *steps);

/* ---- make_beams: many launchers in one call; failed entries reported ---------
 * make_beam (src/solve.jl:209-242) for n_beams launchers at once, the five-call
 * sequence torj_launch_peripheral_rays per launcher, torj_ray_entry_beams*_gpu,
 * torj_trace_beams*, torj_shell_volumes as one entry point.  Unlike the
 * reference's @assert (src/solve.jl:138,141) a ray that fails the ray entry does
 * not end the call: it is reported, per beam, and the rays that entered are
 * traced -- a candidate angle of a steering or density scan whose beam grazes or
 * misses the plasma is an outcome, not an error.
 *
 * Launch (host): per launcher N0 = torj_pol_tor_angles_2_vector(pol, tor),
 * x0 = (r cos phi, r sin phi, z), omega = 2 pi f, and the rays of
 * torj_launch_peripheral_rays(x0, N0, spot_size, inverse_curvature_radius, f,
 * N_rings, min_azimuthal_points, normalize_weight_sum = 1); the launchers' ray
 * counts may differ.  Entry (GPU) of all n rays, torj_ray_entry_beams[_plasmas]_device.
 * The rays that entered are closed up, launched order kept within each beam, and
 * traced by one torj_trace_beams[_plasmas]_device launch with that call's plans
 * and lanes per ray on the kept counts; their weights are NOT renormalised, so
 * deposited_power is the share of the beam's power that coupled and was absorbed
 * and w_ok says how much coupled.  A beam none of whose rays entered is an empty
 * beam: its row is 0.
 *
 * Plasmas: n_plasmas == 0 and plasmas == NULL send every beam through p; else
 * beam b goes through plasmas[launchers[b].plasma] under the rules of
 * torj_trace_beams_plasmas (p the launching handle).  cfg: omega and mode are
 * ignored (the launchers give them); the rest is torj_trace_beams', with its
 * refusals.  psi_dP_dV: n_psi >= 2 shell boundaries, strictly increasing.
 * Outputs (host, each may be NULL): dP_dV, n_beams x n_psi, row b = row b of
 * torj_trace_beams' dP_shell over the shell volumes of beam b's plasma
 * (torj_shell_volumes), its last entry 0; res, n_beams; ray_off, n_beams + 1, the
 * launched offsets: beam b owns rays ray_off[b] .. ray_off[b + 1] - 1 of every
 * per-ray array; rays, the per-ray arrays over all n = ray_off[n_beams] launched
 * rays, laid out as the single calls lay them out.  A ray that failed entry has
 * status = its entry status (TORJ_RAY_REFLECTED or TORJ_RAY_ENTRY_FAIL), steps 0,
 * P_dep 0 and NaN in state and in its traj columns.
 * With dP_dV, res and rays all NULL and ray_off given the call only counts the
 * rays: the two-call pattern of torj_launch_peripheral_rays.  Then only
 * launchers, n_beams, N_rings and min_azimuthal_points are read; of each launcher
 * f and mode are checked as in the full call, plasma is not.
 *
 * Host pointers, synchronous, checked (torj_trace_check runs inside).  Every
 * argument is checked before any device work; the message starts with
 * "torj_make_beams:" and names the argument, and torj_trace_beams' argument
 * refusals follow, also before any device work.  Its workspace-budget refusal
 * (TORJ_WS_GB) alone needs the device and the kept counts: it comes after the
 * entry has run.  The per-ray device arrays live in a grow-only buffer of the
 * handle p, released with the handle: nothing per ray is allocated per call once
 * it has grown.  It holds every per-ray array twice, launched and kept, both at
 * the launched count (sized once, before the entry): 41 + 10 n_save doubles and
 * 7 ints per launched ray, n_save = n_steps / traj_stride samples when rays->traj
 * is given, else 0 -- for 1 104 rays and 2 000 samples 2 x 88 MB. */
typedef struct {
    double r, phi, z;                              /* make_beam's launch point (src/solve.jl:212-215) */
    double steering_angle_tor, steering_angle_pol;
    double spot_size, inverse_curvature_radius;
    double f;                                      /* Hz */
    int mode;                                      /* +1 X, -1 O */
    int plasma;                                    /* index into plasmas[]; unused when n_plasmas == 0 */
} torj_launcher;

typedef struct {
    int n_rays, n_ok;                 /* rays launched; rays that passed entry */
    int first_bad_ray, first_bad_status; /* within the beam; -1, 0 when n_ok == n_rays */
    double w_ok;                      /* sum of the launched weights of the rays that entered */
    double deposited_power;           /* make_beam's (dP_shell[n_psi] of the beam's row) */
} torj_beam_result;

typedef struct {   /* all host arrays, each may be NULL; n = sum of n_rays, launched order */
    double *pos, *dir, *weights;      /* 3 x n, 3 x n, n: launch_peripheral_rays' outputs */
    double *x_plasma, *N_plasma, *s0; /* ray entry's */
    int *entry_status;
    double *state; int *status, *steps; double *P_dep; double *traj;  /* torj_trace_beams' */
} torj_beams_rays;

int torj_make_beams(torj_plasma_t p, int n_plasmas, const torj_plasma_t *plasmas,
                    int n_beams, const torj_launcher *launchers, int N_rings,
                    int min_azimuthal_points, const torj_trace_cfg *cfg, int n_psi,
                    const double *psi_dP_dV, double *dP_dV, torj_beam_result *res,
                    int *ray_off, const torj_beams_rays *rays);

/* make_beam's fan-out and reduce across the GPUs of this process
 * (src/solve.jl:209-240: one task per ray, then sum_i w_i dP_dV_i and
 * sum_i w_i P_i).  Host pointers, the arguments and outputs of torj_trace_ex.
 * The rays are cut into n_shards contiguous shards (0: automatic -- each
 * device's share in pieces of at most 131 072 rays, at least one per device;
 * otherwise at least n_gpus), their boundaries on 64-ray multiples, dealt
 * round-robin to n_gpus devices: device (p's device + k) mod the device count
 * for k < n_gpus, each with its own copy of the plasma, stream and host thread.
 * A device runs its shards in turn through pinned staging in two slots on a
 * copy stream: shard j + 1's upload and shard j - 1's download overlap shard
 * j's trace (one torj_trace_check after the last), its
 * dP_shell partial accumulating on the device; the partials are summed over
 * the devices by one RCCL all-reduce of n_psi + 1 fp64 (single-process
 * communicator from ncclCommInitAll, kept on the handle; n_gpus = 1 needs no
 * reduce unless env TORJ_BEAM_RCCL=1).  Per-ray outputs equal torj_trace_ex's
 * for the same rays and scheduling; dP_shell differs by summation order only.
 * Errors name the failing device.  Test-only: env TORJ_BEAM_SAME_DEVICE=1 puts
 * every replica on p's own device (the threaded multi-replica branch on one
 * GPU; the partials are then summed on the host, RCCL refusing a device twice). */
int torj_trace_beam(torj_plasma_t p, const torj_trace_cfg *cfg, int n, const double *x0,
                    const double *N0, const double *weights, int n_psi, const double *psi_grid,
                    const double *x_launch, const double *s0, double *state, int *status,
                    int *steps, double *dP_shell, double *P_dep, double *traj, int n_gpus,
                    int n_shards);

/* make_beam's fan-out over DEVICE-RESIDENT shards (the serving / benchmark
 * form of torj_trace_beam: inputs already in HBM, no host staging).  Shard k
 * lives on replica k's device -- (p's device + k) mod the device count -- and
 * its pointers are that device's memory, laid out exactly as the arguments of
 * torj_trace_device_ex.  Each replica traces its shard on its own stream from
 * its own host thread (n = 0: nothing), waits and checks it (torj_trace_check);
 * then, with deposition (n_psi >= 2, psi_grid and dP_shell on every shard),
 * the (n_psi + 1) dP_shell vectors are all-reduced in place by RCCL, so every
 * shard's dP_shell holds the sum over the shards (zero them first: the trace
 * accumulates into them).  n_gpus = 1 skips the reduce unless env
 * TORJ_BEAM_RCCL=1.  Synchronous.  Same reference interface as torj_trace_beam
 * (src/solve.jl:209-240). */
typedef struct {
    int n;                                    /* rays in this shard */
    const double *x0, *N0;                    /* 3 x n */
    const double *weights;                    /* n or NULL */
    const double *psi_grid;                   /* n_psi (this device's copy) */
    const double *x_launch, *s0;              /* 3 x n, n (deposition = 1) or NULL */
    double *state;                            /* 7 x n */
    int *status, *steps;                      /* n */
    double *dP_shell;                         /* n_psi + 1, accumulated, then all-reduced */
    double *P_dep;                            /* n or NULL */
    double *traj;                             /* (n_steps / traj_stride) x 5 x n or NULL */
    uint64_t *counters;                       /* 8 or NULL (torj_trace_device) */
} torj_beam_shard;
int torj_trace_beam_device(torj_plasma_t p, const torj_trace_cfg *cfg, int n_gpus, int n_psi,
                           const torj_beam_shard *shards);

/* Scheduling of torj_trace / torj_trace_device launches on this plasma handle
 * (no reference counterpart: an MI355X tuning knob; results are independent
 * of it up to the summation order of dP_shell).  mode -1: default (env
 * TORJ_SCHED; else 1 when the beam has more
 * 64-ray groups than the device has SIMDs, otherwise 0); 0: one lane per ray for the whole trace; 1: persistent
 * waves pulling 64-ray groups chunk by chunk from a ready queue; 2: the whole
 * trace with 16 lanes per ray (Albajar absorption, no binning: the node pairs
 * of the absorption integral split between a ray's lanes, results equal to
 * rounding; mode -1 picks it for beams of at most 2 x 64 x SIMDs / 16 rays
 * unless env TORJ_LPR=1); 3: the split RK4 path (fixed steps, Albajar or
 * warm absorption): the trajectories' cold RK4 in one kernel, the 4 x n_steps
 * alpha evaluations per ray in a fully parallel one, the optical depth by an
 * in-order scan, blocks of steps pipelined over two streams (DESIGN.md 3.7;
 * mode -1 picks it for Albajar where it would pick 1, for the weakly
 * relativistic warm model always and for the fully relativistic one on beams
 * of fewer than 3 x 64-ray groups per CU, unless env TORJ_SPLIT=0;
 * TORJ_SPLIT_WARM=0 / 1 turns the warm choice off / on for every size).
 * waves: number of persistent waves for mode 1 (0 = default: min(8 per CU, G - G/16));
 * steps per pipeline block for mode 3 (0 = from the 1 GiB per alpha-input
 * buffer budget, env TORJ_SPLIT_MB; four buffers in flight). */
int torj_set_sched(torj_plasma_t p, int mode, int waves);

/* Waits for `stream` and checks every trace launched on this handle since
 * the previous check (the flags are sticky: each launch ORs its outcome in,
 * this call reads and clears them): that each psi_dP_dV grid was strictly
 * increasing (checked on the device, so the _device calls never read device
 * memory back or synchronise inside the launch; the host-pointer calls also
 * check their host copy up front), and for work-queue launches, that every ray
 * group retired and the stall watchdog (no progress anywhere in the grid for
 * 120 s) did not fire.  torj_trace[_ex] call it themselves; callers of the
 * asynchronous _device calls call it before trusting the outputs.  All
 * _device calls on one handle must use one stream: they share the handle's
 * scratch (work queue, deposition workspace). */
int torj_trace_check(torj_plasma_t p, void *stream);

/* Per-phase HIP-event timing of torj_trace[_device][_ex] calls on this handle
 * (measurement support, no reference counterpart).  torj_timing(p, 1) clears
 * and enables recording: events on the call's stream before the trace kernel,
 * after it, and after the deposition kernels.  torj_timing_read waits for the
 * recorded calls and returns their count and summed trace-kernel / post-
 * processing milliseconds, then clears. */
int torj_timing(torj_plasma_t p, int enable);
int torj_timing_read(torj_plasma_t p, int *calls, double *trace_ms, double *post_ms);

/* The same per replica of a torj_trace_beam[_device] fan-out (torj_timing(p, 1)
 * enables it on the handle and every replica): calls, trace_ms, post_ms are
 * arrays of n_gpus entries (replica k = device (p's device + k) mod count; k = 0
 * is p), each as torj_timing_read returns it, and reduce_ms the summed host-
 * clock time of make_beam's RCCL all-reduce (the grouped ncclAllReduce and its
 * stream waits).  Clears what it reads. */
int torj_beam_timing_read(torj_plasma_t p, int n_gpus, int *calls, double *trace_ms, double *post_ms,
                          double *reduce_ms);

/* Who took part in make_beam's reduce (src/solve.jl:233-240) of the last
 * torj_trace_beam[_device] fan-out over n_gpus replicas (measurement support,
 * no reference counterpart): per replica k, the HIP device it ran on
 * (device[k]), and its RCCL communicator's rank count (ncclCommCount) and
 * rank (ncclCommUserRank) in nranks[k] / rank[k] -- or 0 / -1 where no
 * communicator exists (one replica without TORJ_BEAM_RCCL=1: nothing to
 * reduce; the test-only same-device placement: partials summed on the host).  Arrays of n_gpus
 * entries; n_gpus may not exceed the handle's replicas. */
int torj_beam_comm_info(torj_plasma_t p, int n_gpus, int *device, int *nranks, int *rank);

/* power_deposition_profile(plasma, s, x, dP_ds, psi_dP_dV) (src/plasma.jl:91-151)
 * on the GPU for n_rays rays at once: ray r has n_points[r] >= 4 points with
 * strictly increasing s, concatenated ray after ray -- s and dP_ds (sum of
 * n_points), x component-major 3 x (sum of n_points).  psi at each point from
 * the plasma's psi spline; the not-a-knot cubic fits of psi(s) - psi_j and
 * dP/ds (Dierckx.Spline1D k = 3), their roots (Dierckx.roots, maxn = 8: the
 * first 8 per boundary in s order), the |integral| per root pair and the
 * outside-in walk, as torj_trace_ex's deposition = 1 applies to a trace.
 * Outputs: dP_dV n_rays x n_psi, row r = ray r's dP_dV (its last entry 0, as
 * the reference's), and P (n_rays).  Host pointers, synchronous.  Errors
 * mirror the reference's: too few points or non-increasing s (Dierckx), a
 * non-increasing psi_dP_dV. */
int torj_power_deposition_profile(torj_plasma_t p, int n_rays, const int *n_points, const double *s,
                                  const double *x, const double *dP_ds, int n_psi,
                                  const double *psi_dP_dV, double *dP_dV, double *P);

/* shell volumes dV[j] = V(psi_grid[j+1]) - V(psi_grid[j]), j < n_psi-1 (host;
 * src/plasma.jl:117-122) */
int torj_shell_volumes(torj_plasma_t p, int n_psi, const double *psi_grid, double *dV);

#ifdef __cplusplus
}
#endif
#endif /* TORJ_HIP_H */
