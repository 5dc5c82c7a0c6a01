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

--plasmas P1,P2,...: the same beams through differing plasmas.  24 beams, beam b through
plasma b mod P of P synthetic tokamaks of differing Te0 and ne_scale:
  (a) P torj_trace_beams_device calls in sequence on one stream, one per plasma with
      that plasma's beams -- the only way before torj_trace_beams_plasmas_device;
  (b) one torj_trace_beams_plasmas_device call, launched by plasma 0's handle.
With P = 1 (a) is the existing call on the same tables, so the pair shows what the
plasma table costs.  The outputs of (a) and (b) must be the same bits (asserted).

    python tools/beams_bench.py --plasmas 1,2,8,24 --out profiles/r12/beams_plasmas_bench.json
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
    ap.add_argument("--plasmas", default=None, help="plasma counts, e.g. 1,2,8,24: the multi-plasma comparison")
    args = ap.parse_args()
    if args.plasmas:
        return main_plasmas(args)

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


N_BEAMS_PL = 24


def main_plasmas(args):
    import torch

    torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import torj_hip as T
    from torj_hip import synthetic as S

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    L, lib = T.lib(), T._lib
    T.abs_Al_init(24)
    s = S.SETUP
    grid = np.linspace(0.0, 1.0, N_PSI)
    B = N_BEAMS_PL

    def t(a, dtype=torch.float64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype=dtype)

    def timed(fn, handles):
        """fn enqueues on `handles`; wall ms around the sync, torj_timing's trace and post ms summed over them"""
        for h in handles:
            lib.check(L.torj_timing(h.handle, 1))
        stream.synchronize()
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        tot = dict(wall_ms=wall, trace_ms=0.0, post_ms=0.0, calls=0)
        for h in handles:
            calls, tr, po = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
            lib.check(L.torj_timing_read(h.handle, ctypes.byref(calls), ctypes.byref(tr), ctypes.byref(po)))
            lib.check(L.torj_timing(h.handle, 0))
            lib.check(L.torj_trace_check(h.handle, stream.cuda_stream))
            tot["trace_ms"] += tr.value  # (torj_timing_read: sums over the handle's calls)
            tot["post_ms"] += po.value
            tot["calls"] += calls.value
        return tot

    fans, omega, mode = [], [], []
    for k in range(B):
        f, m, pol, tor = KINDS[k % len(KINDS)]
        N0 = T.pol_tor_angles_2_vector(np.deg2rad(pol), np.deg2rad(tor))
        fans.append(T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"],
                                             s["inverse_curvature_radius"], f))
        omega.append(2 * np.pi * f)
        mode.append(m)
    d_grid = t(grid)
    cfg = lib.TraceCfg(0.0, 0, DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, 0, 1)

    class Launch:
        """the beams `which` (indices into the 24) as one multi-beam launch: tables, inputs, outputs"""

        def __init__(self, which, ent):
            self.which = which
            cnt = [len(fans[k][2]) for k in which]
            self.off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
            self.om = np.array([omega[k] for k in which])
            self.md = np.array([mode[k] for k in which], dtype=np.int32)
            n = self.n = int(self.off[-1])
            cat = lambda key: np.concatenate([ent[k][key] for k in which])  # noqa: E731
            self.i = dict(x0=t(cat("xp").T), N0=t(cat("Np").T), w=t(cat("w")), xl=t(cat("pos").T), s0=t(cat("s0")))
            self.o = dict(state=torch.empty((7, n), dtype=torch.float64, device=dev),
                          status=torch.empty(n, dtype=torch.int32, device=dev),
                          steps=torch.empty(n, dtype=torch.int32, device=dev),
                          dP=torch.zeros((len(which), N_PSI + 1), dtype=torch.float64, device=dev),
                          Pdep=torch.empty(n, dtype=torch.float64, device=dev))

        def tail(self):
            i, o = self.i, self.o
            return (cfg, len(self.which), lib.iptr(self.off), lib.dptr(self.om), lib.iptr(self.md),
                    i["x0"].data_ptr(), i["N0"].data_ptr(), i["w"].data_ptr(), N_PSI, d_grid.data_ptr(),
                    i["xl"].data_ptr(), i["s0"].data_ptr(), o["state"].data_ptr(), o["status"].data_ptr(),
                    o["steps"].data_ptr(), o["dP"].data_ptr(), o["Pdep"].data_ptr(), None, None, stream.cuda_stream)

    results = []
    for P in (int(v) for v in args.plasmas.split(",")):
        hs = [T.Plasma(*S.plasma_args(S.circular_tokamak(Te0=1500.0 + 200.0 * j, ne_scale=0.6 + 0.03 * j)), device=0)
              for j in range(P)]
        bp = np.array([k % P for k in range(B)], dtype=np.int32)
        handles = lib.handles(hs)
        # every beam entered into its own plasma, in one launch
        off = np.concatenate([[0], np.cumsum([len(fan[2]) for fan in fans])])
        pos, dirs, w = (np.concatenate([fan[k] for fan in fans]) for k in range(3))
        xp, Np, s0, st = T.ray_entry_beams(hs[0], off, omega, mode, pos, dirs, plasmas=hs, beam_plasma=bp)
        assert (st == 0).all()
        ent = [dict(pos=pos[off[k]:off[k + 1]], w=w[off[k]:off[k + 1]], xp=xp[off[k]:off[k + 1]],
                    Np=Np[off[k]:off[k + 1]], s0=s0[off[k]:off[k + 1]]) for k in range(B)]
        whole = Launch(list(range(B)), ent)
        per = [Launch([k for k in range(B) if k % P == j], ent) for j in range(P)]

        def run_a():
            for j in range(P):
                per[j].o["dP"].zero_()
                lib.check(L.torj_trace_beams_device(hs[j].handle, *per[j].tail()))

        def run_b():
            whole.o["dP"].zero_()
            lib.check(L.torj_trace_beams_plasmas_device(hs[0].handle, P, handles, lib.iptr(bp), *whole.tail()))

        timed(run_a, hs), timed(run_b, hs[:1])  # warm-up: allocations, code objects, the handles' device state
        same = True
        for j in range(P):
            for q, k in enumerate(per[j].which):
                lo, hi = int(per[j].off[q]), int(per[j].off[q + 1])
                for key in ("state", "status", "steps", "Pdep"):
                    same &= torch.equal(whole.o[key][..., off[k]:off[k + 1]], per[j].o[key][..., lo:hi])
                same &= torch.equal(whole.o["dP"][k], per[j].o["dP"][q])
        assert same, f"P={P}: the outputs of (a) and (b) differ"
        pairs = [dict(a=timed(run_a, hs), b=timed(run_b, hs[:1])) for _ in range(args.pairs)]
        ratios = [p["a"]["wall_ms"] / p["b"]["wall_ms"] for p in pairs]
        mid = pairs[len(pairs) // 2]
        results.append(dict(n_plasmas=P, n_beams=B, n_rays=int(off[-1]), outputs_equal=bool(same), pairs=pairs,
                            wall_ratio_a_over_b=ratios,
                            middle_pair_trace_plus_post_ms=dict(
                                a=mid["a"]["trace_ms"] + mid["a"]["post_ms"], b=mid["b"]["trace_ms"] + mid["b"]["post_ms"]),
                            b_faster_in_every_pair=all(r > 1.0 for r in ratios)))
        print(f"P={P:3d} beams={B} rays={int(off[-1])} equal={same} " + " ".join(
            f"[a {p['a']['wall_ms']:.2f} b {p['b']['wall_ms']:.2f} ms]" for p in pairs), flush=True)
        if P >= 2:
            assert results[-1]["b_faster_in_every_pair"], f"P={P}: one launch is not faster in every pair"

    doc = dict(tool="tools/beams_bench.py --plasmas", build_id=L.torj_build_id().decode(),
               device=torch.cuda.get_device_name(0), n_steps=N_STEPS, ds=DS, chunk_steps=CHUNK, n_psi=N_PSI,
               absorption="albajar", deposition="reference", rays_per_beam=46, n_beams=B,
               plasmas="beam b through plasma b mod P; plasma j: Te0 = 1500 + 200 j eV, ne_scale = 0.6 + 0.03 j",
               a="P torj_trace_beams_device calls in sequence on one stream, one per plasma (baseline; "
                 "P = 1: the existing call on the same tables)",
               b="one torj_trace_beams_plasmas_device call", results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(dict(beams_plasmas_bench=[dict(n_plasmas=r["n_plasmas"], wall_ratio=r["wall_ratio_a_over_b"])
                                               for r in results])))


if __name__ == "__main__":
    main()
