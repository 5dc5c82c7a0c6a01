#!/usr/bin/env python3
"""Wall time of torj_ray_profile_device beside torj_trace_beams_device on the same rays
(device-resident inputs, one stream, each call followed by torj_trace_check): a warm pair,
then `--pairs` alternating pairs.  The rays are those of tests/test_gpu_ray_profile.py: 32
rays of five beams, 12 000 steps of 1e-4 m, a row / trajectory sample every 1 000 steps.
Prints one JSON line.  Informational: no threshold."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torj.jl_amd"))

DS, N_STEPS, CHUNK, STRIDE = 1e-4, 12000, 120, 1000
BEAMS = ((92.5e9, 1, 30.0, 0.0, 13), (92.5e9, -1, 30.0, 0.0, 5), (140e9, 1, 30.0, 0.0, 0),
         (110e9, 1, 30.0, 0.0, 1), (85.5e9, -1, 25.0, 5.0, 13))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--sched", type=int, default=-1, help="torj_set_sched mode (-1 automatic, 0 one lane, 2 sixteen)")
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    import torj_hip as T
    from torj_hip import synthetic as S
    from torj_hip._lib import TraceCfg, check, dptr, iptr

    T.abs_Al_init(24)
    P = T.Plasma(*S.plasma_args(S.circular_tokamak()))
    P.set_sched(args.sched)
    s = S.SETUP
    xp, Np, s0, off, omega, mode = [], [], [], [0], [], []
    for f, m, pol, tor, k in BEAMS:
        N0 = T.pol_tor_angles_2_vector(np.deg2rad(pol), np.deg2rad(tor))
        pos, dirs, _ = T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"],
                                                s["inverse_curvature_radius"], f)
        x, N, sv, st = T.ray_entry(P, pos, dirs, 2 * np.pi * f, m)
        assert (st == 0).all()
        xp.append(x[:k]), Np.append(N[:k]), s0.append(sv[:k])
        off.append(off[-1] + k), omega.append(2 * np.pi * f), mode.append(m)
    off, omega, mode = np.array(off, dtype=np.int32), np.array(omega), np.array(mode, dtype=np.int32)
    n, nb, n_rows = int(off[-1]), len(omega), N_STEPS // STRIDE + 1
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=torch.float64)
    x0, N0d, s0d = t(np.concatenate(xp).T), t(np.concatenate(Np).T), t(np.concatenate(s0))
    state = torch.empty((7, n), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    steps = torch.empty(n, dtype=torch.int32, device=dev)
    prof = torch.empty((n_rows, 25, n), dtype=torch.float64, device=dev)
    traj = torch.empty((n_rows - 1, 5, n), dtype=torch.float64, device=dev)
    cfg = TraceCfg(0.0, 0, DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, STRIDE)
    L = T.lib()
    tables = (nb, iptr(off), dptr(omega), iptr(mode))
    outs = (state.data_ptr(), status.data_ptr(), steps.data_ptr())

    def profile():
        check(L.torj_ray_profile_device(P.handle, 0, None, None, cfg, *tables, x0.data_ptr(), N0d.data_ptr(),
                                        s0d.data_ptr(), n_rows, prof.data_ptr(), *outs, stream))

    def trace():
        check(L.torj_trace_beams_device(P.handle, cfg, *tables, x0.data_ptr(), N0d.data_ptr(), None, 0, None, None,
                                        s0d.data_ptr(), *outs, None, None, traj.data_ptr(), None, stream))

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        check(L.torj_trace_check(P.handle, stream))
        return (time.perf_counter() - t0) * 1e3

    timed(profile), timed(trace)  # the warm pair
    pairs = [(timed(profile), timed(trace)) for _ in range(args.pairs)]
    # the two phases of one profile call (torj_timing): the trace, then the point kernel
    L.torj_timing(P.handle, 1)
    profile()
    calls, tr, post = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
    check(L.torj_timing_read(P.handle, ctypes.byref(calls), ctypes.byref(tr), ctypes.byref(post)))
    L.torj_timing(P.handle, 0)
    print(json.dumps(dict(metric="ray_profile_wall_ms", rays=n, steps=N_STEPS, rows=n_rows, sched=args.sched,
                          build_id=L.torj_build_id().decode(),
                          pairs_profile_vs_trace_beams_ms=[[round(a, 3), round(b, 3)] for a, b in pairs],
                          profile_trace_kernel_ms=round(tr.value, 3), profile_point_kernel_ms=round(post.value, 3))))


if __name__ == "__main__":
    main()
