#!/usr/bin/env python
"""Many small beams: one launch per beam against one launch for all.

B beams of the default 46-ray fan from SETUP's launch point, their frequency,
mode and steering cycling through tests/test_gpu_beams.py's five, 2 000 steps
of 1e-4 m with Albajar absorption and the reference deposition on 1 000
shells, inputs device-resident.  Timed, alternating, after a warm-up pair:
  (a) B torj_trace_device_ex calls in sequence on one stream -- the only way to
      trace such a system before torj_trace_beams_device, hence the baseline;
  (b) one torj_trace_beams_device call.
Each reports the wall time around a stream synchronisation and torj_timing's
trace / post milliseconds.  The outputs of (a) and (b) are compared once per B
(they are the same bits).  Writes one JSON document, stamped with the build id.

    python tools/beams_bench.py --out profiles/r09/beams_bench.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "torj.jl_amd"))

# frequency, mode, steering pol / tor (degrees): tests/test_gpu_beams.py's non-empty beams
KINDS = ((92.5e9, 1, 30.0, 0.0), (92.5e9, -1, 30.0, 0.0), (110e9, 1, 30.0, 0.0), (100e9, 1, 35.0, -5.0),
         (85.5e9, -1, 25.0, 5.0))
DS, N_STEPS, CHUNK, N_PSI = 1e-4, 2000, 20, 1000


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--beams", default="1,8,24,96")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import torj_hip as T
    from torj_hip import synthetic as S

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    L, lib = T.lib(), T._lib
    P = T.Plasma(*S.plasma_args(S.circular_tokamak()), device=0)
    T.abs_Al_init(24)
    s = S.SETUP
    grid = np.linspace(0.0, 1.0, N_PSI)

    def t(a, dtype=torch.float64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dtype)

    def timed(fn):
        """fn enqueues; wall ms around the sync, torj_timing's trace and post ms"""
        lib.check(L.torj_timing(P.handle, 1))
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        calls, tr, po = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        lib.check(L.torj_timing_read(P.handle, ctypes.byref(calls), ctypes.byref(tr), ctypes.byref(po)))
        lib.check(L.torj_timing(P.handle, 0))
        lib.check(L.torj_trace_check(P.handle, stream.cuda_stream))
        return dict(wall_ms=wall, trace_ms=tr.value, post_ms=po.value, calls=calls.value)

    results = []
    for B in (int(v) for v in args.beams.split(",")):
        fans, off, omega, mode = [], [0], [], []
        for k in range(B):
            f, m, pol, tor = KINDS[k % len(KINDS)]
            N0 = T.pol_tor_angles_2_vector(np.deg2rad(pol), np.deg2rad(tor))
            fans.append(T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"],
                                                 s["inverse_curvature_radius"], f))
            off.append(off[-1] + len(fans[-1][2]))
            omega.append(2 * np.pi * f)
            mode.append(m)
        pos, dirs, w = (np.concatenate([fan[k] for fan in fans]) for k in range(3))
        xp, Np, s0, st = T.ray_entry_beams(P, off, omega, mode, pos, dirs)
        assert (st == 0).all()
        n = off[-1]
        off_a, om_a, md_a = np.array(off, dtype=np.int32), np.array(omega), np.array(mode, dtype=np.int32)
        # per-ray arrays are component-major over all n rays for (b); (a) gets each beam's own copy
        d_grid = t(grid)

        def outputs(nr, nb):
            return dict(state=torch.empty((7, nr), dtype=torch.float64, device=dev),
                        status=torch.empty(nr, dtype=torch.int32, device=dev),
                        steps=torch.empty(nr, dtype=torch.int32, device=dev),
                        dP=torch.zeros((nb, N_PSI + 1), dtype=torch.float64, device=dev),
                        Pdep=torch.empty(nr, dtype=torch.float64, device=dev))

        def inputs(sl):
            return dict(x0=t(xp[sl].T), N0=t(Np[sl].T), w=t(w[sl]), xl=t(pos[sl].T), s0=t(s0[sl]))

        all_in, all_out = inputs(slice(0, n)), outputs(n, B)
        per = [(inputs(slice(off[k], off[k + 1])), outputs(off[k + 1] - off[k], 1)) for k in range(B)]
        cfgs = [lib.TraceCfg(omega[k], mode[k], DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, 0, 1) for k in range(B)]
        cfg = lib.TraceCfg(0.0, 0, DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, 0, 1)

        def run_a():
            for k in range(B):
                i, o = per[k]
                o["dP"].zero_()
                lib.check(L.torj_trace_device_ex(
                    P.handle, cfgs[k], off[k + 1] - off[k], i["x0"].data_ptr(), i["N0"].data_ptr(), i["w"].data_ptr(),
                    N_PSI, d_grid.data_ptr(), i["xl"].data_ptr(), i["s0"].data_ptr(), o["state"].data_ptr(),
                    o["status"].data_ptr(), o["steps"].data_ptr(), o["dP"].data_ptr(), o["Pdep"].data_ptr(), None,
                    None, stream.cuda_stream))

        def run_b():
            i, o = all_in, all_out
            o["dP"].zero_()
            lib.check(L.torj_trace_beams_device(
                P.handle, cfg, B, lib.iptr(off_a), lib.dptr(om_a), lib.iptr(md_a), i["x0"].data_ptr(),
                i["N0"].data_ptr(), i["w"].data_ptr(), N_PSI, d_grid.data_ptr(), i["xl"].data_ptr(),
                i["s0"].data_ptr(), o["state"].data_ptr(), o["status"].data_ptr(), o["steps"].data_ptr(),
                o["dP"].data_ptr(), o["Pdep"].data_ptr(), None, None, stream.cuda_stream))

        timed(run_a), timed(run_b)  # warm-up: allocations, code objects
        same = all(
            torch.equal(all_out[key][..., off[k]:off[k + 1]] if key != "dP" else all_out[key][k:k + 1], per[k][1][key])
            for k in range(B) for key in ("state", "status", "steps", "dP", "Pdep"))
        pairs = [dict(a=timed(run_a), b=timed(run_b)) for _ in range(args.pairs)]
        ratios = [p["a"]["wall_ms"] / p["b"]["wall_ms"] for p in pairs]
        results.append(dict(n_beams=B, n_rays=n, outputs_equal=bool(same), pairs=pairs, wall_ratio_a_over_b=ratios,
                            trace_ratio_a_over_b=[p["a"]["trace_ms"] / p["b"]["trace_ms"] for p in pairs],
                            b_faster_in_every_pair=all(r > 1.0 for r in ratios)))
        print(f"B={B:3d} rays={n:5d} equal={same} " + " ".join(
            f"[a {p['a']['wall_ms']:.2f} b {p['b']['wall_ms']:.2f} ms]" for p in pairs), flush=True)

    doc = dict(tool="tools/beams_bench.py", build_id=L.torj_build_id().decode(),
               device=torch.cuda.get_device_name(0), n_steps=N_STEPS, ds=DS, chunk_steps=CHUNK, n_psi=N_PSI,
               absorption="albajar", deposition="reference", rays_per_beam=46,
               a="B torj_trace_device_ex calls in sequence on one stream (baseline)",
               b="one torj_trace_beams_device call", results=results)
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps(dict(beams_bench=[dict(n_beams=r["n_beams"], wall_ratio=r["wall_ratio_a_over_b"]) for r in results])))


if __name__ == "__main__":
    main()
