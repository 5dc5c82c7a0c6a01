"""make_ray / make_beam (src/solve.jl) on top of the HIP ray-stepping kernel.

Integration semantics (DESIGN.md "Integrator"): fixed-step RK4 with
ds = 1e-4 m (the reference's dtmax, src/solve.jl:157), optical depth tau with
P = exp(-tau), termination checks (psi > 1, P < 1e-6) at the boundaries of the
reference's 100 chunks (src/solve.jl:145,174,176), and psi-shell deposition
binned in-kernel.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import (BeamResult, BeamsRays, Launcher, TraceCfg, TorjError, check, dptr, f64, handles, iptr, lib,
                   soa)
from .launch import launch_peripheral_rays, pol_tor_angles_2_vector

OK, LEFT_PLASMA, ABSORBED, NAN, REFLECTED, ENTRY_FAIL, MAX_STEPS = range(7)
STATUS_NAMES = ("OK", "LEFT_PLASMA", "ABSORBED", "NAN", "REFLECTED", "ENTRY_FAIL", "MAX_STEPS")


class RayEntryError(AssertionError):
    """The reference's @assert failures in first_point/make_ray (src/solve.jl:32,138,141)
    and its unhandled reflection return (src/solve.jl:57-59)."""


def ray_entry(plasma, x0, N0, omega: float, mode: int, *, gpu: bool = False):
    """first_point + vacuum_plasma_refraction for a batch (src/solve.jl:7-74).
    Returns (x_plasma (n,3), N_plasma (n,3), s0 (n,), status (n,)).  gpu=True
    runs the one-lane-per-ray HIP kernel (torj_ray_entry_gpu); the default is
    the host C++ path (OpenMP), usable without a GPU."""
    xs, Ns = soa(x0), soa(N0)
    n = xs.shape[1]
    xp, Np = np.zeros((3, n)), np.zeros((3, n))
    s0 = np.zeros(n)
    st = np.zeros(n, dtype=np.int32)
    fn = lib().torj_ray_entry_gpu if gpu else lib().torj_ray_entry
    check(fn(plasma.handle, n, dptr(xs), dptr(Ns), float(omega), int(mode), dptr(xp), dptr(Np),
             dptr(s0), iptr(st)))
    return xp.T.copy(), Np.T.copy(), s0, st


@dataclass
class TraceResult:
    state: np.ndarray     # (n, 7): x, y, z, Nx, Ny, Nz, tau
    status: np.ndarray    # (n,)
    steps: np.ndarray     # (n,)
    dP_shell: np.ndarray  # (n_psi + 1,): sum_rays w * dP per shell, [n_psi] = sum w * P_dep
    P_dep: np.ndarray     # (n,)
    traj: np.ndarray | None  # (n, n_save, 5): x, y, z, tau, s

    @property
    def P_end(self):
        return np.exp(-self.state[:, 6])


DEPOSITION = {"binned": 0, "reference": 1}
INTEGRATOR = {"rk4": 0, "adaptive": 1}
ABSORPTION = {"none": 0, "albajar": 1, "warm_wr": 2, "warm_fr": 3}


def _absorption_code(absorption) -> int:
    """bool (True = Albajar, the reference's abs_Albajar_fast), a name from
    ABSORPTION, or the ABI integer 0..3."""
    if isinstance(absorption, str):
        return ABSORPTION[absorption]
    if isinstance(absorption, (bool, np.bool_)):
        return int(bool(absorption))
    a = int(absorption)
    if a not in (0, 1, 2, 3):
        raise ValueError(f"absorption must be 0..3, got {a}")
    return a


def trace(plasma, x0, N0, omega: float, mode: int, *, ds: float = 1e-4, n_steps: int,
          chunk_steps: int | None = None, psi_exit: float = 1.0, P_min: float = 1e-6,
          absorption=True, psi_grid=None, weights=None, traj_stride: int = 0,
          deposition: str = "binned", x_launch=None, s0=None, integrator: str = "rk4",
          abstol: float = 1e-6, reltol: float = 1e-6, s_max: float | None = None,
          n_chunks: int = 100, n_gpus: int | None = None, n_shards: int = 0) -> TraceResult:
    """Integrate rays from in-plasma start states (x0, N0: (n, 3)) on the GPU.

    deposition="binned": psi-shell binning of every step (P_dep = 1 - P_end per
    ray); "reference": power_deposition_profile's FITPACK semantics
    (src/plasma.jl:91-151) from make_ray's saved points, which needs the
    vacuum launch points x_launch (n, 3) and path lengths s0 (n,).

    integrator="rk4": n_steps fixed steps of ds; "adaptive": the reference's
    solve() -- Tsit5 with DiffEq's step control (abstol, reltol, dtmax = ds) over
    n_chunks tspans covering s_max from s0; n_steps is then the accepted-step
    capacity per ray (status MAX_STEPS when exceeded).

    n_gpus: None traces on the plasma's device (torj_trace_ex); an integer runs
    make_beam's multi-GPU path (torj_trace_beam): n_shards contiguous shards
    (0: one per GPU) over n_gpus devices, dP_shell summed by an RCCL all-reduce."""
    xs, Ns = soa(x0), soa(N0)
    n = xs.shape[1]
    if chunk_steps is None:
        chunk_steps = max(1, n_steps // 100)
    dmode = DEPOSITION[deposition]
    imode = INTEGRATOR[integrator]
    cfg = TraceCfg(float(omega), int(mode), float(ds), int(n_steps), int(chunk_steps),
                   float(psi_exit), float(P_min), _absorption_code(absorption), int(traj_stride), dmode,
                   imode, float(abstol), float(reltol),
                   float(s_max if s_max is not None else n_steps * ds), int(n_chunks))
    xl = soa(x_launch) if x_launch is not None else None
    sv = f64(s0) if s0 is not None else None
    g = f64(psi_grid) if psi_grid is not None else np.zeros(0)
    n_psi = len(g)
    w = f64(weights) if weights is not None else None
    state = np.zeros((7, n))
    status = np.zeros(n, dtype=np.int32)
    steps = np.zeros(n, dtype=np.int32)
    dP = np.zeros(n_psi + 1)
    Pdep = np.zeros(n)
    n_save = n_steps // traj_stride if traj_stride > 0 else 0
    traj = np.zeros((n_save, 5, n)) if n_save > 0 else None
    args = (plasma.handle, cfg, n, dptr(xs), dptr(Ns), dptr(w), n_psi, dptr(g) if n_psi else None,
            dptr(xl), dptr(sv), dptr(state), iptr(status), iptr(steps), dptr(dP), dptr(Pdep),
            dptr(traj))
    if n_gpus is None:
        check(lib().torj_trace_ex(*args))
    else:
        check(lib().torj_trace_beam(*args, int(n_gpus), int(n_shards)))
    return TraceResult(state.T.copy(), status, steps, dP, Pdep,
                       traj.transpose(2, 0, 1).copy() if traj is not None else None)


def _steps_for(s_max: float, ds: float) -> int:
    return max(1, int(round(s_max / ds)))


def _beam_tables(beam_off, omega, mode):
    """The three host tables of a multi-beam call: beam b owns rays
    beam_off[b] .. beam_off[b + 1] - 1 and is traced with omega[b], mode[b]."""
    off = np.ascontiguousarray(beam_off, dtype=np.int32)
    om = f64(omega)
    md = np.ascontiguousarray(mode, dtype=np.int32)
    if off.ndim != 1 or om.ndim != 1 or md.ndim != 1 or len(om) != len(md) or len(off) != len(om) + 1:
        raise ValueError("beam_off needs n_beams + 1 entries, omega and mode n_beams each")
    return off, om, md


def _plasma_tables(plasmas, beam_plasma, n_beams):
    """The two further host tables of a call through several plasmas: the listed
    handles and beam b's index into them (both or neither)."""
    if plasmas is None and beam_plasma is None:
        return None
    if plasmas is None or beam_plasma is None:
        raise ValueError("plasmas and beam_plasma go together")
    bp = np.ascontiguousarray(beam_plasma, dtype=np.int32)
    if bp.ndim != 1 or len(bp) != n_beams:
        raise ValueError("beam_plasma needs n_beams entries")
    return len(plasmas), handles(plasmas), iptr(bp), bp


def ray_entry_beams(plasma, beam_off, omega, mode, x0, N0, *, plasmas=None, beam_plasma=None):
    """ray_entry(..., gpu=True) for the concatenated rays of several beams, ray i
    with its beam's omega and mode, in one launch (torj_ray_entry_beams_gpu).
    With plasmas (a sequence of Plasma) and beam_plasma (n_beams indices into it)
    beam b enters plasmas[beam_plasma[b]], with that plasma's own psi_prof_max
    (torj_ray_entry_beams_plasmas_gpu); `plasma` is then the launching handle."""
    off, om, md = _beam_tables(beam_off, omega, mode)
    pt = _plasma_tables(plasmas, beam_plasma, len(om))
    xs, Ns = soa(x0), soa(N0)
    n = xs.shape[1]
    if len(off) and off[-1] != n:
        raise ValueError(f"beam_off[-1] = {off[-1]}, but {n} rays given")
    xp, Np = np.zeros((3, n)), np.zeros((3, n))
    s0 = np.zeros(n)
    st = np.zeros(n, dtype=np.int32)
    args = (len(om), iptr(off), dptr(om), iptr(md), dptr(xs), dptr(Ns), dptr(xp), dptr(Np), dptr(s0), iptr(st))
    if pt is None:
        check(lib().torj_ray_entry_beams_gpu(plasma.handle, *args))
    else:
        check(lib().torj_ray_entry_beams_plasmas_gpu(plasma.handle, *pt[:3], *args))
    return xp.T.copy(), Np.T.copy(), s0, st


def trace_beams(plasma, beam_off, omega, mode, x0, N0, *, ds: float = 1e-4, n_steps: int,
                chunk_steps: int | None = None, psi_exit: float = 1.0, P_min: float = 1e-6,
                absorption=True, psi_grid=None, weights=None, traj_stride: int = 0,
                deposition: str = "binned", x_launch=None, s0=None, plasmas=None,
                beam_plasma=None) -> TraceResult:
    """trace() for the concatenated rays of several beams in ONE launch
    (torj_trace_beams): beam b owns rays beam_off[b] .. beam_off[b + 1] - 1 and
    is traced with omega[b] and mode[b]; every other setting is shared.
    dP_shell has shape (n_beams, n_psi + 1), row b beam b's.  Fixed-step RK4 with
    absorption "none" or "albajar" only; per-ray results equal trace()'s on each
    beam alone.

    plasmas (a sequence of Plasma on `plasma`'s device) and beam_plasma (n_beams
    indices into it): beam b is traced through plasmas[beam_plasma[b]]
    (torj_trace_beams_plasmas) and its results equal trace()'s on that plasma;
    `plasma` is then the launching handle (its set_sched knobs, stream and scratch),
    listed or not.  The grids of the plasmas may differ."""
    off, om, md = _beam_tables(beam_off, omega, mode)
    pt = _plasma_tables(plasmas, beam_plasma, len(om))
    xs, Ns = soa(x0), soa(N0)
    n = xs.shape[1]
    if len(off) and off[-1] != n:
        raise ValueError(f"beam_off[-1] = {off[-1]}, but {n} rays given")
    if chunk_steps is None:
        chunk_steps = max(1, n_steps // 100)
    cfg = TraceCfg(0.0, 0, float(ds), int(n_steps), int(chunk_steps), float(psi_exit), float(P_min),
                   _absorption_code(absorption), int(traj_stride), DEPOSITION[deposition])
    xl = soa(x_launch) if x_launch is not None else None
    sv = f64(s0) if s0 is not None else None
    g = f64(psi_grid) if psi_grid is not None else np.zeros(0)
    n_psi = len(g)
    w = f64(weights) if weights is not None else None
    state = np.zeros((7, n))
    status = np.zeros(n, dtype=np.int32)
    steps = np.zeros(n, dtype=np.int32)
    dP = np.zeros((len(om), n_psi + 1))
    Pdep = np.zeros(n)
    n_save = n_steps // traj_stride if traj_stride > 0 else 0
    traj = np.zeros((n_save, 5, n)) if n_save > 0 else None
    args = (cfg, len(om), iptr(off), dptr(om), iptr(md), dptr(xs), dptr(Ns), dptr(w), n_psi,
            dptr(g) if n_psi else None, dptr(xl), dptr(sv), dptr(state), iptr(status), iptr(steps), dptr(dP),
            dptr(Pdep), dptr(traj))
    if pt is None:
        check(lib().torj_trace_beams(plasma.handle, *args))
    else:
        check(lib().torj_trace_beams_plasmas(plasma.handle, *pt[:3], *args))
    return TraceResult(state.T.copy(), status, steps, dP, Pdep,
                       traj.transpose(2, 0, 1).copy() if traj is not None else None)


# the columns of a ray profile's rows, in the order of include/torj_hip.h's TORJ_PROF_* enum
PROFILE_COLUMNS = ("x", "y", "z", "Nx", "Ny", "Nz", "tau", "s", "P", "alpha", "dP_ds", "psi", "ne", "Te",
                   "Bx", "By", "Bz", "B_abs", "X", "Y", "N_par", "N_abs", "Ns2", "Lambda", "dLambda_dN")


@dataclass
class RayProfile:
    table: np.ndarray   # (n, n_rows, 25): row k of ray i is step k * traj_stride, NaN where the ray had stopped
    state: np.ndarray   # (n, 7), status (n,), steps (n,): trace_beams' outputs
    status: np.ndarray
    steps: np.ndarray
    columns = PROFILE_COLUMNS

    def __getitem__(self, name):
        """column `name` over all rays and rows, (n, n_rows)"""
        return self.table[:, :, self.columns.index(name)]


def ray_profile(plasma, beam_off, omega, mode, x0, N0, *, s0=None, plasmas=None, beam_plasma=None,
                ds: float = 1e-4, n_steps: int, chunk_steps: int | None = None, traj_stride: int,
                absorption=True, psi_exit: float = 1.0, P_min: float = 1e-6) -> RayProfile:
    """N, the plasma parameters and alpha at every saved point of the rays of several
    beams (torj_ray_profile): the rays are traced as trace_beams traces them without
    deposition, and row k of ray i holds, at step k * traj_stride (row 0: the entry
    point), the PROFILE_COLUMNS: x, N, tau, s, P, alpha_approx, dP/ds = P alpha, psi_norm,
    n_e, T_e, B, |B|, X, Y, N_par, |N|, the cold refractive_index_sq, the dispersion
    relation Lambda and |dLambda/dN|.  Rows beyond a ray's last step are NaN.  s0
    (n,): arc lengths at the entry points (None: s counts from there).  plasmas and
    beam_plasma as in trace_beams.  A warm alpha along the ray is one further call:
    alpha_warm(omega, r["X"], r["Y"], r["N_abs"], r["N_par"], r["Te"], 1 / r["dLambda_dN"], mode)."""
    off, om, md = _beam_tables(beam_off, omega, mode)
    pt = _plasma_tables(plasmas, beam_plasma, len(om))
    xs, Ns = soa(x0), soa(N0)
    n = xs.shape[1]
    if len(off) and off[-1] != n:
        raise ValueError(f"beam_off[-1] = {off[-1]}, but {n} rays given")
    if chunk_steps is None:
        chunk_steps = max(1, n_steps // 100)
    cfg = TraceCfg(0.0, 0, float(ds), int(n_steps), int(chunk_steps), float(psi_exit), float(P_min),
                   _absorption_code(absorption), int(traj_stride))
    sv = f64(s0) if s0 is not None else None
    n_rows = n_steps // traj_stride + 1 if traj_stride > 0 else 0
    prof = np.zeros((max(n_rows, 0), len(PROFILE_COLUMNS), n))
    state = np.zeros((7, n))
    status = np.zeros(n, dtype=np.int32)
    steps = np.zeros(n, dtype=np.int32)
    sel = pt[:3] if pt is not None else (0, None, None)
    check(lib().torj_ray_profile(plasma.handle, *sel, cfg, len(om), iptr(off), dptr(om), iptr(md), dptr(xs),
                                 dptr(Ns), dptr(sv), n_rows, dptr(prof), dptr(state), iptr(status), iptr(steps)))
    return RayProfile(prof.transpose(2, 0, 1).copy(), state.T.copy(), status, steps)


def make_ray(plasma, x0, N_vacuum, f: float, mode: int, s_max: float, psi_dP_dV, *,
             ds: float = 1e-4, deposition: str = "reference", integrator: str = "rk4",
             max_steps: int | None = None, absorption="albajar"):
    """make_ray (src/solve.jl:135-181) -> (s, u, P_beam, dP_dV_ray, deposited_power).
    deposition="reference" (default) follows power_deposition_profile; "binned"
    uses the in-kernel shell binning.  integrator="adaptive" runs the reference's
    solve() semantics (Tsit5, dtmax = ds, 100 chunks); "rk4" fixed steps of ds.
    absorption: "albajar" (alpha_approx, the reference's), "warm_wr" / "warm_fr"
    (general_absorption.jl's alpha, iwarm 1 / 3) or "none"."""
    omega = 2.0 * np.pi * f
    x0 = f64(x0)
    xp, Np, s0, st = ray_entry(plasma, x0[None], f64(N_vacuum)[None], omega, mode)
    if st[0] != OK:
        raise RayEntryError(f"ray entry failed: {STATUS_NAMES[st[0]]}")
    n_steps = _steps_for(s_max, ds)
    if integrator == "adaptive":
        n_steps = max_steps or 2 * n_steps + 400
    g = f64(psi_dP_dV)
    r = trace(plasma, xp, Np, omega, mode, ds=ds, n_steps=n_steps, psi_grid=g, traj_stride=1,
              deposition=deposition, x_launch=x0[None], s0=s0, integrator=integrator, s_max=s_max,
              absorption=absorption)
    if r.status[0] == MAX_STEPS:
        raise RuntimeError("make_ray: accepted-step capacity exhausted (raise max_steps)")
    k = int(r.steps[0])
    s = np.concatenate([[0.0, s0[0]], r.traj[0, :k, 4]])
    u = np.vstack([x0[None], xp, r.traj[0, :k, :3]])
    P_beam = np.concatenate([[1.0, 1.0], np.exp(-r.traj[0, :k, 3])])
    dV = plasma.shell_volumes(g)
    dP_dV = np.zeros(len(g))
    dP_dV[:-1] = r.dP_shell[:len(g) - 1] / dV
    return s, u, P_beam, dP_dV, float(r.P_dep[0])


def fma(a: float, b: float, c: float) -> float:
    """a * b + c with ONE rounding (Python 3.10 has no math.fma): the exact
    rational value, rounded once by the correctly rounded Fraction -> float."""
    from fractions import Fraction

    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _final_arc_length(res, i, s0, ds):
    """Arc length of ray i's final RK4 state: fma(steps, ds, s0), the single-
    rounding product-sum the trajectory kernel stores (its s0 + steps * ds is
    contracted to one v_fma_f64)."""
    return fma(float(int(res.steps[i])), float(ds), float(s0))


def _ray_lists(res, rays, pos, xp, s0, ds, traj_stride):
    """make_beam's per-ray lists (arc lengths, trajectories, powers) of the rays
    `rays` of a TraceResult: the launch point, the entry point, the saved samples
    and, where it is not one of them, the final state."""
    arc_lengths, trajectories, ray_powers = [], [], []
    for i in rays:
        k = int(res.steps[i]) // traj_stride
        s_i, x_i, tau_i = res.traj[i, :k, 4], res.traj[i, :k, :3], res.traj[i, :k, 3]
        if int(res.steps[i]) % traj_stride:  # the final state is not a saved sample
            s_end = _final_arc_length(res, i, s0[i], ds)
            s_i = np.concatenate([s_i, [s_end]])
            x_i = np.vstack([x_i, res.state[i, :3][None]])
            tau_i = np.concatenate([tau_i, [res.state[i, 6]]])
        arc_lengths.append(np.concatenate([[0.0, s0[i]], s_i]))
        trajectories.append(np.vstack([pos[i][None], xp[i][None], x_i]))
        ray_powers.append(np.concatenate([[1.0, 1.0], np.exp(-tau_i)]))
    return arc_lengths, trajectories, ray_powers


def make_beam(plasma, r: float, phi: float, z: float, steering_angle_tor: float,
              steering_angle_pol: float, spot_size: float, inverse_curvature_radius: float,
              f: float, mode: int, s_max: float, psi_dP_dV, *, ds: float = 1e-4,
              traj_stride: int = 1, deposition: str = "reference", integrator: str = "rk4",
              max_steps: int | None = None, absorption="albajar", n_gpus: int = 1, **kwargs):
    """make_beam (src/solve.jl:209-242) -> (arc_lengths, trajectories, ray_powers, dP_dV,
    deposited_power, ray_weights).  kwargs go to launch_peripheral_rays.  The rays
    are traced by torj_trace_beam over n_gpus devices of this process (the
    reference's per-ray Dagger tasks, src/solve.jl:219-224) and their deposition
    summed across them (:233-240).  traj_stride > 1 keeps every traj_stride-th
    step of each ray plus its final state, so ray_powers[i][-1] is the ray's
    final P as in the reference."""
    if integrator == "adaptive" and traj_stride > 1:
        # checked before any tracing: the adaptive integrator's final state is
        # not a saved sample and its arc length is not recorded
        raise ValueError("make_beam: integrator='adaptive' needs traj_stride = 1")
    omega = 2.0 * np.pi * f
    N0 = pol_tor_angles_2_vector(steering_angle_pol, steering_angle_tor)
    x0 = np.array([r * np.cos(phi), r * np.sin(phi), z])
    pos, dirs, w = launch_peripheral_rays(x0, N0, spot_size, inverse_curvature_radius, f, **kwargs)
    xp, Np, s0, st = ray_entry(plasma, pos, dirs, omega, mode, gpu=True)
    bad = np.flatnonzero(st != OK)
    if len(bad):
        raise RayEntryError(f"{len(bad)} rays failed entry, first: ray {bad[0]} "
                            f"{STATUS_NAMES[st[bad[0]]]}")
    n_steps = _steps_for(s_max, ds)
    if integrator == "adaptive":
        n_steps = max_steps or 2 * n_steps + 400
    g = f64(psi_dP_dV)
    res = trace(plasma, xp, Np, omega, mode, ds=ds, n_steps=n_steps, psi_grid=g, weights=w,
                traj_stride=traj_stride, deposition=deposition, x_launch=pos, s0=s0,
                integrator=integrator, s_max=s_max, absorption=absorption, n_gpus=n_gpus)
    if (res.status == MAX_STEPS).any():
        raise RuntimeError("make_beam: accepted-step capacity exhausted (raise max_steps)")
    dV = plasma.shell_volumes(g)
    dP_dV = np.zeros(len(g))
    dP_dV[:-1] = res.dP_shell[:len(g) - 1] / dV
    deposited_power = float(res.dP_shell[len(g)])
    arc_lengths, trajectories, ray_powers = _ray_lists(res, range(len(w)), pos, xp, s0, ds, traj_stride)
    return arc_lengths, trajectories, ray_powers, dP_dV, deposited_power, w


def make_beams(plasma, launchers, s_max: float, psi_dP_dV, *, ds: float = 1e-4, traj_stride: int = 1,
               deposition: str = "reference", absorption="albajar", plasmas=None, beam_plasma=None, **kwargs):
    """make_beam for several launchers in ONE launch (torj_ray_entry_beams_gpu,
    torj_trace_beams): `launchers` is a sequence of (r, phi, z, steering_angle_tor,
    steering_angle_pol, spot_size, inverse_curvature_radius, f, mode), make_beam's
    leading arguments; returns one make_beam tuple per launcher, equal to what
    make_beam gives for it.  Fixed-step RK4, absorption "albajar" or "none";
    kwargs go to launch_peripheral_rays.  Raises RayEntryError naming the beam
    when a ray fails entry.  With plasmas and beam_plasma (see trace_beams)
    launcher b goes through plasmas[beam_plasma[b]] and its tuple equals
    make_beam's on that plasma, dP_dV taken with that plasma's shell volumes."""
    fans, omega, mode, off = [], [], [], [0]
    for (r, phi, z, tor, pol, spot, inv_curv, f, m) in launchers:
        N0 = pol_tor_angles_2_vector(pol, tor)
        x0 = np.array([r * np.cos(phi), r * np.sin(phi), z])
        fans.append(launch_peripheral_rays(x0, N0, spot, inv_curv, f, **kwargs))
        omega.append(2.0 * np.pi * f)
        mode.append(int(m))
        off.append(off[-1] + len(fans[-1][2]))
    pos, dirs, w = (np.concatenate([fan[k] for fan in fans]) for k in range(3))
    sel = dict(plasmas=plasmas, beam_plasma=beam_plasma)
    xp, Np, s0, st = ray_entry_beams(plasma, off, omega, mode, pos, dirs, **sel)
    for b in range(len(fans)):
        bad = np.flatnonzero(st[off[b]:off[b + 1]] != OK)
        if len(bad):
            raise RayEntryError(f"beam {b}: {len(bad)} rays failed entry, first: ray {bad[0]} "
                                f"{STATUS_NAMES[st[off[b] + bad[0]]]}")
    g = f64(psi_dP_dV)
    res = trace_beams(plasma, off, omega, mode, xp, Np, ds=ds, n_steps=_steps_for(s_max, ds), psi_grid=g,
                      weights=w, traj_stride=traj_stride, deposition=deposition, x_launch=pos, s0=s0,
                      absorption=absorption, **sel)
    # the shells' volumes: the launching plasma's, or each listed plasma's own
    dV = [q.shell_volumes(g) for q in plasmas] if plasmas is not None else [plasma.shell_volumes(g)]
    out = []
    for b in range(len(fans)):
        dP_dV = np.zeros(len(g))
        dP_dV[:-1] = res.dP_shell[b, :len(g) - 1] / dV[beam_plasma[b] if plasmas is not None else 0]
        lists = _ray_lists(res, range(off[b], off[b + 1]), pos, xp, s0, ds, traj_stride)
        out.append((*lists, dP_dV, float(res.dP_shell[b, len(g)]), w[off[b]:off[b + 1]]))
    return out


def _launcher_table(launchers, beam_plasma):
    la = (Launcher * len(launchers))()
    for b, (r, phi, z, tor, pol, spot, inv_curv, f, m) in enumerate(launchers):
        la[b] = Launcher(float(r), float(phi), float(z), float(tor), float(pol), float(spot), float(inv_curv),
                         float(f), int(m), int(beam_plasma[b]) if beam_plasma is not None else 0)
    return la


def make_beams_arrays(plasma, launchers, s_max: float, psi_dP_dV, *, ds: float = 1e-4, traj_stride: int = 1,
                      deposition: str = "reference", absorption="albajar", plasmas=None, beam_plasma=None,
                      N_rings: int = 3, min_azimuthal_points: int = 5) -> dict:
    """torj_make_beams as it is, two calls (the ray count, then the arrays): a dict of
    `off` (n_beams + 1 launched offsets), `results` (n_beams dicts of torj_beam_result's
    fields), `dP_dV` (n_beams, n_psi), the launch's `pos`, `dirs` (n, 3) and `w` (n,),
    the entry's `xp`, `Np` (n, 3), `s0` and `entry_status` (n,), and `res`, a
    TraceResult over all n launched rays (dP_shell None), all in launched order."""
    if (plasmas is None) != (beam_plasma is None):
        raise ValueError("plasmas and beam_plasma go together")
    B = len(launchers)
    if beam_plasma is not None and len(beam_plasma) != B:
        raise ValueError("beam_plasma needs n_beams entries")
    la = _launcher_table(launchers, beam_plasma)
    hs, n_pl = (handles(plasmas), len(plasmas)) if plasmas is not None else (None, 0)
    n_steps = _steps_for(s_max, ds)
    cfg = TraceCfg(0.0, 0, float(ds), n_steps, max(1, n_steps // 100), 1.0, 1e-6, _absorption_code(absorption),
                   int(traj_stride), DEPOSITION[deposition])
    g = f64(psi_dP_dV)
    off = np.zeros(B + 1, dtype=np.int32)
    head = (plasma.handle, n_pl, hs, B, la, int(N_rings), int(min_azimuthal_points), cfg, len(g), dptr(g))
    rc = lib().torj_make_beams(*head, None, None, iptr(off), None)
    if rc != 0 and lib().torj_last_error().decode().startswith("ArgumentError"):
        raise ValueError(lib().torj_last_error().decode())
    check(rc)
    n = int(off[B])
    n_save = n_steps // traj_stride if traj_stride > 0 else 0
    a = dict(pos=np.zeros((3, n)), dir=np.zeros((3, n)), weights=np.zeros(n), x_plasma=np.zeros((3, n)),
             N_plasma=np.zeros((3, n)), s0=np.zeros(n), entry_status=np.zeros(n, dtype=np.int32),
             state=np.zeros((7, n)), status=np.zeros(n, dtype=np.int32), steps=np.zeros(n, dtype=np.int32),
             P_dep=np.zeros(n), traj=np.zeros((n_save, 5, n)) if n_save > 0 else None)
    rays = BeamsRays(*[iptr(a[k]) if k in ("entry_status", "status", "steps") else dptr(a[k])
                       for k, _ in BeamsRays._fields_])
    dP_dV = np.zeros((B, len(g)))
    res = (BeamResult * B)()
    check(lib().torj_make_beams(*head, dptr(dP_dV), res, iptr(off), rays))
    traj = a["traj"].transpose(2, 0, 1).copy() if a["traj"] is not None else None
    return dict(off=off, dP_dV=dP_dV, results=[{k: getattr(r, k) for k, _ in BeamResult._fields_} for r in res],
                pos=a["pos"].T.copy(), dirs=a["dir"].T.copy(), w=a["weights"], xp=a["x_plasma"].T.copy(),
                Np=a["N_plasma"].T.copy(), s0=a["s0"], entry_status=a["entry_status"],
                res=TraceResult(a["state"].T.copy(), a["status"], a["steps"], None, a["P_dep"], traj))


def make_beams_c(plasma, launchers, s_max: float, psi_dP_dV, *, ds: float = 1e-4, traj_stride: int = 1,
                 deposition: str = "reference", absorption="albajar", plasmas=None, beam_plasma=None,
                 N_rings: int = 3, min_azimuthal_points: int = 5):
    """make_beams through the one C entry point torj_make_beams -> (tuples, results).
    tuples[b] is make_beam's 6-tuple of launcher b built from the call's per-ray
    arrays; where every ray enters it equals make_beams'.  A ray that fails entry
    does not raise: the per-ray lists of tuples[b] (arc lengths, trajectories, ray
    powers, weights) are over the rays that entered, with their launched weights
    (not renormalised), and results[b] holds torj_beam_result's fields: n_rays,
    n_ok, first_bad_ray and first_bad_status within the beam (-1, 0 when all
    entered), w_ok, deposited_power."""
    m = make_beams_arrays(plasma, launchers, s_max, psi_dP_dV, ds=ds, traj_stride=traj_stride,
                          deposition=deposition, absorption=absorption, plasmas=plasmas, beam_plasma=beam_plasma,
                          N_rings=N_rings, min_azimuthal_points=min_azimuthal_points)
    off, st = m["off"], m["entry_status"]
    tuples = []
    for b, r in enumerate(m["results"]):
        ok = off[b] + np.flatnonzero(st[off[b]:off[b + 1]] == OK)
        lists = _ray_lists(m["res"], ok, m["pos"], m["xp"], m["s0"], ds, traj_stride)
        tuples.append((*lists, m["dP_dV"][b].copy(), float(r["deposited_power"]), m["w"][ok]))
    return tuples, m["results"]
