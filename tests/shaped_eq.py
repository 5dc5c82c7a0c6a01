"""A shaped test equilibrium and the launches traced through it (helper module of
tests/test_gpu_geometry.py and tests/test_oracle_symmetry.py; generated, no fixture).

synthetic.circular_tokamak() is an exact quadratic psi without an R-Z cross term,
up-down symmetric, on a square box with hR == hZ, and every test launches from
the low-field side at phi = 0.  shaped_tokamak() has none of these properties:

  x = (R - R0 - 0.06) / a,  y = (Z + 0.05) / (kappa a),  kappa = 1.6
  psi = x^2 + y^2 + 0.25 x y^2 + 0.08 y^3 exp(-x^2) + 0.05 x^3  - (its grid minimum)
  B_R = -sigma Psi_a / R dpsi/dZ,  B_Z = sigma Psi_a / R dpsi/dR,  B_phi = sigma B0 R0 / R

(non-polynomial, a mixed derivative, shifted, up-down asymmetric; sigma = -1
reverses the whole field) on a 40 x 61 box R in [0.95, 2.65], Z in [-1.25, 1.15]:
hR = 0.0436 != hZ = 0.04, asymmetric about Z = 0, and (nR + 2)(nZ + 2) 48 B =
127 008 B, so that the whole-grid LDS trajectory kernel still takes it."""
import numpy as np
from torj_hip import synthetic as S

KAPPA = 1.6
NR, NZ = 40, 61
R_RANGE, Z_RANGE = (0.95, 2.65), (-1.25, 1.15)
F = 92.5e9
OMEGA = 2 * np.pi * F
PHI_ROT = 2.3  # |y| ~ 1.1 |x| for a launch from phi = 0

# name -> launch point, steering pol / tor in degrees
LAUNCHES = {
    "lfs_down": ((2.6, 0.0, -0.6), -25.0, -12.0),
    "top": ((1.8, 0.0, 1.1), 85.0, 15.0),
    "hfs": ((1.0, 0.0, 0.1), 170.0, 5.0),
}
# the launch of the entry finding (test_oracle_symmetry.py test_entry_does_not_depend_on_the_toroidal_angle)
EDGE_LAUNCH = ((2.6, 0.0, 0.45), 30.0, 8.0)


def shaped_tokamak(sigma=1.0, Te0=3000.0, nR=NR, nZ=NZ, R_range=R_RANGE, Z_range=Z_RANGE, n_prof=101,
                   n_eq=101, ne0=3e19, ne_edge=1e17, Te_edge=30.0):
    """The 11 inputs of Plasma(...) as a dict (synthetic.plasma_args turns it into the tuple)."""
    a = S.A_MINOR
    R = np.linspace(R_range[0], R_range[1], nR)
    Z = np.linspace(Z_range[0], Z_range[1], nZ)
    RR, ZZ = np.meshgrid(R, Z, indexing="ij")
    x = (RR - S.R0 - 0.06) / a
    y = (ZZ + 0.05) / (KAPPA * a)
    e = np.exp(-x * x)
    psi = x * x + y * y + 0.25 * x * y * y + 0.08 * y ** 3 * e + 0.05 * x ** 3
    psi_x = 2.0 * x + 0.25 * y * y - 0.16 * x * y ** 3 * e + 0.15 * x * x
    psi_y = 2.0 * y + 0.5 * x * y + 0.24 * y * y * e
    psi = psi - psi.min()
    Br = -sigma * (S.PSI_A / RR) * psi_y / (KAPPA * a)
    Bz = sigma * (S.PSI_A / RR) * psi_x / a
    Bphi = sigma * S.B0 * S.R0 / RR
    psi_prof = np.linspace(0.0, 1.0, n_prof)
    ne_prof = ne0 * (1.0 - psi_prof) + ne_edge
    Te_prof = Te0 * (1.0 - psi_prof) ** 2 + Te_edge
    eq_psi = np.linspace(0.0, 1.0, n_eq)
    eq_vol = 2.0 * np.pi ** 2 * S.R0 * KAPPA * a ** 2 * eq_psi
    return dict(R_coords=R, Z_coords=Z, psi_norm_data=psi, psi_prof=psi_prof, ne_prof=ne_prof,
                Te_prof=Te_prof, Br_data=Br, Bz_data=Bz, Bphi_data=Bphi, eqt1d_psi_norm=eq_psi,
                eqt1d_volume=eq_vol)


def shaped_args(**kw):
    return S.plasma_args(shaped_tokamak(**kw))


def rotz(v, phi):
    """(n, 3) vectors rotated about the Z axis by phi"""
    v = np.asarray(v, dtype=float)
    c, s = np.cos(phi), np.sin(phi)
    return np.stack([c * v[..., 0] - s * v[..., 1], s * v[..., 0] + c * v[..., 1], v[..., 2]], -1)


def mirror(v):
    """(n, 3) vectors mirrored in the plane Z = 0"""
    return np.asarray(v, dtype=float) * np.array([1.0, 1.0, -1.0])


def mirror_image(eq):
    """The mirror image in Z = 0 of an equilibrium dict whose psi, B_Z and B_phi are even
    and whose B_R is odd in Z on a box symmetric about Z = 0 (circular_tokamak()): B is a
    pseudovector, so the image has the toroidal field reversed and is otherwise the same."""
    out = dict(eq)
    out["Bphi_data"] = -eq["Bphi_data"]
    return out


def fan(M, launch, n_rings=3, min_az=5, phi=0.0, f=F):
    """launch_peripheral_rays of module M (torj_hip or the oracle) for a LAUNCHES entry,
    then rotated about Z by phi, positions and directions alike: (pos, dirs, weights)"""
    x0, pol, tor = launch
    s = S.SETUP
    N0 = M.pol_tor_angles_2_vector(np.deg2rad(pol), np.deg2rad(tor))
    pos, dirs, w = M.launch_peripheral_rays(list(x0), N0, s["spot_size"], s["inverse_curvature_radius"], f,
                                            N_rings=n_rings, min_azimuthal_points=min_az)
    if phi:
        pos, dirs = rotz(pos, phi), rotz(dirs, phi)
    return pos, dirs, w


def trace_errs(state, ref, tau_floor=1e-6):
    """worst relative x, N and (floored) tau differences of two (n, 7) state arrays:
    _compare_trace's three figures (tests/test_gpu_parity.py)"""
    ex = np.abs(state[:, :3] - ref[:, :3]).max(1) / np.linalg.norm(ref[:, :3], axis=1)
    eN = np.abs(state[:, 3:6] - ref[:, 3:6]).max(1) / np.linalg.norm(ref[:, 3:6], axis=1)
    et = np.abs(state[:, 6] - ref[:, 6]) / np.maximum(np.abs(ref[:, 6]), tau_floor)
    return ex.max(), eN.max(), et.max()


def rot_state(state, phi):
    """(n, 7) end states with x and N rotated about Z by phi (tau kept)"""
    return np.concatenate([rotz(state[:, :3], phi), rotz(state[:, 3:6], phi), state[:, 6:]], 1)


def mirror_state(state):
    return state * np.array([1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 1.0])
