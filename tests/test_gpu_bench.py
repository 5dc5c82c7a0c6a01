"""bench.py as the driver runs it, on a small fan: a plain run times exactly
--steps steps and prints one line with the headline's figures and none of the
legs that moved behind --full; --dump-outputs writes the last timed step's
outputs, which are those torj_hip.trace returns for the same beam."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("cpu_baseline", "parity", "exact", "library_path", "host_api", "host_api_beam_c4", "ray_entry")
N_RINGS, MIN_AZ, N_STEPS, N_PSI, STRIDE = 10, 5, 1500, 200, 100


def test_plain_run_line_and_dumped_outputs(gpu, T, tmp_path):
    from torj_hip import synthetic as S

    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--n-rings", str(N_RINGS), "--min-az", str(MIN_AZ), "--n-steps", str(N_STEPS),
           "--n-psi", str(N_PSI), "--traj-stride", str(STRIDE), "--dump-outputs", out]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["unit"] == "ray-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert not [k for k in FULL_ONLY if k in d]
    assert d["roofline"]["kernel_ms"] > 0 and d["roofline"]["flop_per_launch"] > 0

    # the same beam through the host-pointer API
    s = S.SETUP
    f = 92.5e9
    om = 2 * np.pi * f
    P = T.Plasma(*S.plasma_args(S.circular_tokamak()), device=0)
    N0 = T.pol_tor_angles_2_vector(s["steering_angle_pol"], s["steering_angle_tor"])
    pos, dirs, w = T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"],
                                            s["inverse_curvature_radius"], f, N_rings=N_RINGS,
                                            min_azimuthal_points=MIN_AZ)
    xp, Np, s0, st = T.ray_entry(P, pos, dirs, om, 1, gpu=True)
    assert (st == 0).all()
    g = T.trace(P, xp, Np, om, 1, ds=1e-4, n_steps=N_STEPS, psi_grid=np.linspace(0.0, 1.0, N_PSI),
                weights=w, traj_stride=STRIDE, deposition="reference", x_launch=pos, s0=s0)
    n = len(w)
    a = {k[:-4]: np.load(os.path.join(out, k)) for k in os.listdir(out)}
    assert sorted(a) == ["P_dep", "dP_shell", "ray_index", "state", "status", "steps", "traj"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["ray_index"], np.arange(n))  # a small beam: every ray
    assert d["config"]["rays_per_gpu"] == n
    # value's numerator: the ray-steps of one pass over the beam
    assert abs(d["value"] * d["ms_per_step"] / 1e3 / g.steps.sum() - 1) < 1e-9
    assert np.array_equal(a["status"], g.status) and np.array_equal(a["steps"], g.steps)
    # one library, one device, the same kernels and inputs on both paths
    assert np.array_equal(a["state"], g.state)
    assert np.array_equal(a["traj"], g.traj, equal_nan=True)
    assert np.array_equal(a["P_dep"], g.P_dep)
    # dP_shell is summed over rays by atomics: to rounding
    assert a["dP_shell"].shape == (N_PSI + 1,)
    assert np.abs(a["dP_shell"] - g.dP_shell).max() <= 1e-13 * np.abs(g.dP_shell).max()
