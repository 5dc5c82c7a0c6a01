#!/usr/bin/env python
"""A pool of plasmas refilled: new handles against torj_plasma_update on live ones.

24 plasmas (synthetic tokamaks on G x G nodes, Te0 = 1500 + 200 j eV, ne_scale =
0.6 + 0.03 j) feed one torj_trace_beams_plasmas_device launch: 24 beams of the default
46-ray fan, beam b through plasma b, 2 000 steps of 1e-4 m with Albajar absorption and
the reference deposition on 1 000 shells, rays device-resident (DESIGN.md 3.2d's
workload).  Timed, alternating, after a warm-up pair:
  (a) torj_plasma_destroy + torj_plasma_create of all 24, then the launch -- the only way
      to put new physics on the GPU before torj_plasma_update, hence the baseline;
  (b) torj_plasma_update of the 24 pooled handles on the launch's stream, then the launch;
  (c) torj_plasma_update_gpu of the same handles -- the 2-D prefilters on the device, in the
      stream's order -- then the launch, alternating with (b).
Each reports the wall time from the first refill call to the end of a stream
synchronisation, the host time of the refill calls alone, and torj_timing's trace / post
milliseconds of the launch.  The launch's outputs are the same bits in (a) and (b)
(asserted), and (b) must be faster than (a) in every pair (asserted).  (b) and (c) give the
same bits on the pool and on the split leg (asserted); at 129 x 129 (c) must be faster than
(b) in every pair of the pool leg (asserted), the other figures are recorded.

Also one handle on the split path (torj_set_sched(p, 3, 0), 4 096 rays, 2 000 steps): (a)
destroy + create + trace, (b) update + trace; there the cell table an update builds on the
device differs from the host's in rounding, and the largest output difference is recorded.

Last, one 129 x 129 handle in a profiles-only loop: torj_plasma_update_profiles against
torj_plasma_update_profiles_gpu, each followed by a stream synchronisation (recorded).

    python tools/plasma_update_bench.py --out profiles/r16/plasma_update_bench.json
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

DS, N_STEPS, CHUNK, N_PSI = 1e-4, 2000, 20, 1000
N_POOL, N_SPLIT = 24, 4096
F = 92.5e9
OM = 2 * np.pi * F


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", default="56,129")
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
    T.abs_Al_init(24)
    s = S.SETUP
    d_grid = torch.from_numpy(np.linspace(0.0, 1.0, N_PSI)).to(dev)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def fan(n_rings):
        N0 = T.pol_tor_angles_2_vector(s["steering_angle_pol"], s["steering_angle_tor"])
        return T.launch_peripheral_rays([s["R0"], 0.0, s["z0"]], N0, s["spot_size"], s["inverse_curvature_radius"], F,
                                        N_rings=n_rings)

    def destroy(P):
        lib.check(L.torj_plasma_destroy(P._h))
        P._h = None

    def timed(refill, launch, handle_of):
        """refill() then launch() on the stream; wall ms to the end of the sync, the refill's host ms,
        torj_timing's trace and post ms of the launch"""
        stream.synchronize()
        t0 = time.perf_counter()
        refill()
        t1 = time.perf_counter()
        h = handle_of()
        lib.check(L.torj_timing(h.handle, 1))
        launch()
        stream.synchronize()
        t2 = time.perf_counter()
        calls, tr, po = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        lib.check(L.torj_timing_read(h.handle, ctypes.byref(calls), ctypes.byref(tr), ctypes.byref(po)))
        lib.check(L.torj_timing(h.handle, 0))
        lib.check(L.torj_trace_check(h.handle, stream.cuda_stream))
        return dict(wall_ms=(t2 - t0) * 1e3, refill_host_ms=(t1 - t0) * 1e3, trace_ms=tr.value, post_ms=po.value,
                    calls=calls.value)

    def outputs(n, rows):
        return dict(state=torch.empty((7, n), dtype=torch.float64, device=dev),
                    status=torch.empty(n, dtype=torch.int32, device=dev),
                    steps=torch.empty(n, dtype=torch.int32, device=dev),
                    dP=torch.zeros((rows, N_PSI + 1), dtype=torch.float64, device=dev),
                    Pdep=torch.empty(n, dtype=torch.float64, device=dev))

    def pairs_of(run_a, run_b, out, what):
        run_a(), run_b()  # warm-up: allocations, code objects, device state
        keep = {k: v.clone() for k, v in out.items()}
        run_a()
        diff = {k: float((out[k].double() - keep[k].double()).abs().max()) for k in out}  # (a) against (b)
        pairs = [dict(a=run_a(), b=run_b()) for _ in range(args.pairs)]
        ratios = [p["a"]["wall_ms"] / p["b"]["wall_ms"] for p in pairs]
        print(what + " " + " ".join(f"[a {p['a']['wall_ms']:.1f} (refill {p['a']['refill_host_ms']:.1f}) "
                                    f"b {p['b']['wall_ms']:.1f} (refill {p['b']['refill_host_ms']:.1f}) ms]"
                                    for p in pairs), flush=True)
        assert all(r > 1.0 for r in ratios), f"{what}: the update is not faster in every pair"
        return dict(pairs=pairs, wall_ratio_a_over_b=ratios, b_faster_in_every_pair=True,
                    max_abs_output_difference_a_vs_b=diff)

    def pairs_bc(run_b, run_c, out, what, c_must_win):
        """(c) against (b), the same way; their outputs must be the same bits"""
        run_b(), run_c()
        keep = {k: v.clone() for k, v in out.items()}
        run_b()
        diff = {k: float((out[k].double() - keep[k].double()).abs().max()) for k in out}  # (b) against (c)
        assert not any(diff.values()), f"{what}: the outputs differ between (b) and (c): {diff}"
        pairs = [dict(b=run_b(), c=run_c()) for _ in range(args.pairs)]
        ratios = [p["b"]["wall_ms"] / p["c"]["wall_ms"] for p in pairs]
        print(what + " " + " ".join(f"[b {p['b']['wall_ms']:.1f} (refill {p['b']['refill_host_ms']:.1f}) "
                                    f"c {p['c']['wall_ms']:.1f} (refill {p['c']['refill_host_ms']:.1f}) ms]"
                                    for p in pairs), flush=True)
        if c_must_win:
            assert all(r > 1.0 for r in ratios), f"{what}: the device build is not faster in every pair"
        return dict(pairs=pairs, wall_ratio_b_over_c=ratios, c_faster_in_every_pair=all(r > 1.0 for r in ratios),
                    c_faster_asserted=c_must_win, same_bits_b_and_c=True)

    results = []
    for G in (int(v) for v in args.grids.split(",")):
        eqs = [S.circular_tokamak(nR=G, nZ=G, Te0=1500.0 + 200.0 * j, ne_scale=0.6 + 0.03 * j) for j in range(N_POOL)]
        pargs = [S.plasma_args(eq) for eq in eqs]
        hs = [T.Plasma(*a, device=0) for a in pargs]
        # ---- the pool: 24 beams of 46 rays, beam b through plasma b, one launch ----
        pos, dirs, w = fan(3)
        nb = len(w)
        off = (np.arange(N_POOL + 1) * nb).astype(np.int32)
        om, md = np.full(N_POOL, OM), np.ones(N_POOL, dtype=np.int32)
        bp = np.arange(N_POOL, dtype=np.int32)
        cat = lambda v: np.concatenate([v] * N_POOL)  # noqa: E731
        xp, Np, s0, st = T.ray_entry_beams(hs[0], off, om, md, cat(pos), cat(dirs), plasmas=hs, beam_plasma=bp)
        assert (st == 0).all()
        n = int(off[-1])
        i = dict(x0=t(xp.T), N0=t(Np.T), w=t(cat(w)), xl=t(cat(pos).T), s0=t(s0))
        o = outputs(n, N_POOL)
        cfg = lib.TraceCfg(0.0, 0, DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, 0, 1)

        def launch_pool():
            o["dP"].zero_()
            lib.check(L.torj_trace_beams_plasmas_device(
                hs[0].handle, N_POOL, lib.handles(hs), lib.iptr(bp), cfg, N_POOL, lib.iptr(off), lib.dptr(om),
                lib.iptr(md), i["x0"].data_ptr(), i["N0"].data_ptr(), i["w"].data_ptr(), N_PSI, d_grid.data_ptr(),
                i["xl"].data_ptr(), i["s0"].data_ptr(), o["state"].data_ptr(), o["status"].data_ptr(),
                o["steps"].data_ptr(), o["dP"].data_ptr(), o["Pdep"].data_ptr(), None, None, stream.cuda_stream))

        def recreate_pool():
            for j in range(N_POOL):
                destroy(hs[j])
                hs[j] = T.Plasma(*pargs[j], device=0)

        def update_pool():
            for j in range(N_POOL):
                hs[j].update(*pargs[j], stream=stream.cuda_stream or None)

        pool = pairs_of(lambda: timed(recreate_pool, launch_pool, lambda: hs[0]),
                        lambda: timed(update_pool, launch_pool, lambda: hs[0]), o, f"G={G} pool")
        assert not any(pool["max_abs_output_difference_a_vs_b"].values()), "the pool's outputs differ between (a) and (b)"

        def update_pool_gpu():
            for j in range(N_POOL):
                hs[j].update_gpu(*pargs[j], stream=stream.cuda_stream or None)

        pool_bc = pairs_bc(lambda: timed(update_pool, launch_pool, lambda: hs[0]),
                           lambda: timed(update_pool_gpu, launch_pool, lambda: hs[0]), o, f"G={G} pool (b, c)", G == 129)
        # ---- one handle on the split path ----
        pos, dirs, w = (a[:N_SPLIT] for a in fan(34))
        assert len(w) == N_SPLIT
        one = [T.Plasma(*pargs[0], device=0)]
        xp, Np, s0, st = T.ray_entry(one[0], pos, dirs, OM, 1, gpu=True)
        assert (st == 0).all()
        si = dict(x0=t(xp.T), N0=t(Np.T), w=t(w), xl=t(pos.T), s0=t(s0))
        so = outputs(N_SPLIT, 1)
        scfg = lib.TraceCfg(OM, 1, DS, N_STEPS, CHUNK, 1.0, 1e-6, 1, 0, 1)

        def launch_split():
            so["dP"].zero_()
            one[0].set_sched(3, 0)
            lib.check(L.torj_trace_device_ex(
                one[0].handle, scfg, N_SPLIT, si["x0"].data_ptr(), si["N0"].data_ptr(), si["w"].data_ptr(), N_PSI,
                d_grid.data_ptr(), si["xl"].data_ptr(), si["s0"].data_ptr(), so["state"].data_ptr(),
                so["status"].data_ptr(), so["steps"].data_ptr(), so["dP"].data_ptr(), so["Pdep"].data_ptr(), None,
                None, stream.cuda_stream))

        def recreate_one():
            destroy(one[0])
            one[0] = T.Plasma(*pargs[0], device=0)

        def update_one():
            one[0].update(*pargs[0], stream=stream.cuda_stream or None)

        split = pairs_of(lambda: timed(recreate_one, launch_split, lambda: one[0]),
                         lambda: timed(update_one, launch_split, lambda: one[0]), so, f"G={G} split")

        def update_one_gpu():
            one[0].update_gpu(*pargs[0], stream=stream.cuda_stream or None)

        split_bc = pairs_bc(lambda: timed(update_one, launch_split, lambda: one[0]),
                            lambda: timed(update_one_gpu, launch_split, lambda: one[0]), so, f"G={G} split (b, c)", False)
        res = dict(grid=[G, G], pool=dict(n_plasmas=N_POOL, n_beams=N_POOL, n_rays=n, **pool),
                   split=dict(n_rays=N_SPLIT, sched_mode=3, **split), pool_b_vs_c=pool_bc, split_b_vs_c=split_bc)
        if G == 129:  # a transport loop's step: new profiles on one handle, to the end of a synchronisation
            prof = [(eq["psi_prof"], eq["ne_prof"], eq["Te_prof"]) for eq in eqs]

            def loop(call):
                stream.synchronize()
                ms = []
                for j in range(N_POOL):
                    t0 = time.perf_counter()
                    call(*prof[j], stream=stream.cuda_stream or None)
                    t1 = time.perf_counter()
                    stream.synchronize()
                    ms.append(((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3))
                return dict(host_ms_median=float(np.median([m[0] for m in ms[1:]])),
                            to_sync_ms_median=float(np.median([m[1] for m in ms[1:]])), calls=N_POOL - 1)

            loop(one[0].update_profiles), loop(one[0].update_profiles_gpu)  # warm-up
            res["profiles_only_loop"] = dict(update_profiles=loop(one[0].update_profiles),
                                             update_profiles_gpu=loop(one[0].update_profiles_gpu))
            print(f"G={G} profiles-only: {res['profiles_only_loop']}", flush=True)
        results.append(res)
        for P in hs + one:
            destroy(P)

    doc = dict(tool="tools/plasma_update_bench.py", build_id=L.torj_build_id().decode(),
               device=torch.cuda.get_device_name(0), n_steps=N_STEPS, ds=DS, chunk_steps=CHUNK, n_psi=N_PSI,
               absorption="albajar", deposition="reference",
               plasmas="plasma j: Te0 = 1500 + 200 j eV, ne_scale = 0.6 + 0.03 j, on G x G nodes",
               a="torj_plasma_destroy + torj_plasma_create of every handle, then the launch (baseline)",
               b="torj_plasma_update of the live handles on the launch's stream, then the launch",
               c="torj_plasma_update_gpu of the live handles on the launch's stream, then the launch",
               wall_ms="from the first refill call to the end of the stream synchronisation after the launch",
               results=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(dict(plasma_update_bench=[dict(grid=r["grid"], pool=r["pool"]["wall_ratio_a_over_b"],
                                                    split=r["split"]["wall_ratio_a_over_b"],
                                                    pool_b_over_c=r["pool_b_vs_c"]["wall_ratio_b_over_c"],
                                                    split_b_over_c=r["split_b_vs_c"]["wall_ratio_b_over_c"])
                                               for r in results])))


if __name__ == "__main__":
    main()
