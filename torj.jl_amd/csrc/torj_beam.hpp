// torj_beam.hpp -- make_beam across the GPUs of this process: the handle's
// replicas, the RCCL reduction of the shell powers, and the per-replica
// worker that stages, traces and downloads a beam's shards.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include <chrono>
#include <thread>

#include "../../include/torj_hip.h"
#include "torj_plasma.hpp"

// ---- make_beam across the GPUs of this process (src/solve.jl:209-240) -----
// Replica k of a plasma handle: the same coefficients on device (device + k)
// mod the device count, with its own stream, scratch and scheduling copy.
//
// Test-only placement: env TORJ_BEAM_SAME_DEVICE=1 (read per call) puts every
// replica on the handle's own device, so the multi-replica branch -- one host
// thread, stream and workspace per replica -- runs on a one-GPU machine.  RCCL
// rejects a communicator with a device twice, so those partials are summed on
// the host, in replica order, instead of by the all-reduce.
static bool beam_same_device() { return env_int("TORJ_BEAM_SAME_DEVICE", 0) != 0; }

static int beam_replicas(torj_plasma_s *p, int n_gpus, bool same) {
    int ndev = 0;
    HIPCK(hipGetDeviceCount(&ndev));
    if (n_gpus < 1 || (!same && n_gpus > ndev))
        return fail("n_gpus = %d, but %d HIP devices are visible", n_gpus, ndev);
    // a replica that has no device state yet gets it from its host copy of the coefficients: after a
    // device-side build the base handle's copy is downloaded first (mirror_sync), for the new
    // replicas (a changed placement makes them all new) and for those the build found without device state
    auto dev_of = [&](size_t k) { return same ? p->device : (p->device + (int)k) % ndev; };
    bool need = std::max<size_t>(1, p->replicas.size()) < (size_t)n_gpus;
    for (size_t k = 1; k < p->replicas.size(); k++) {
        const torj_plasma_s *q = p->replicas[k];
        need = need || q->device != dev_of(k) || (q->coef_stale && !q->d_flags);
    }
    if (need && mirror_sync(p)) return -1;
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->replicas.empty()) p->replicas.push_back(p);
    for (size_t k = 1; need && k < p->replicas.size(); k++)
        if (p->replicas[k]->coef_stale && !p->replicas[k]->d_flags) {
            p->replicas[k]->coef = p->coef;
            p->replicas[k]->coef_stale = false;
        }
    for (size_t k = 1; k < p->replicas.size(); k++)
        if (p->replicas[k]->device != dev_of(k)) {  // placement changed: rebuild them all
            for (ncclComm_t c : p->comms) (void)ncclCommDestroy(c);
            p->comms.clear();
            for (size_t j = 1; j < p->replicas.size(); j++) torj_plasma_destroy(p->replicas[j]);
            p->replicas.resize(1);
            break;
        }
    while ((int)p->replicas.size() < n_gpus) {
        auto *q = new torj_plasma_s();
        q->device = dev_of(p->replicas.size());
        q->g = p->g;
        q->coef = p->coef;
        q->n_vol = p->n_vol;
        q->v1 = p->v1;
        q->vn = p->vn;
        q->vol_coef = p->vol_coef;
        q->psi_prof_max = p->psi_prof_max;
        q->timing = p->timing;
        p->replicas.push_back(q);
    }
    for (int k = 1; k < n_gpus; k++) {  // scheduling knobs follow the base handle
        p->replicas[k]->sched_mode = p->sched_mode;
        p->replicas[k]->sched_waves = p->sched_waves;
        p->replicas[k]->lanes_per_ray = p->lanes_per_ray;
    }
    return 0;
}

// Run f(k) for k < n_gpus: inline for one replica, else one host thread per
// replica (each drives its own device and stream).  Returns the first failure,
// naming its device.
template <class F>
static int beam_fanout(torj_plasma_s *p, int n_gpus, const char *what, F &&f) {
    std::vector<std::string> errs(n_gpus);
    std::vector<int> rc(n_gpus, 0);
    auto run = [&](int k) {
        rc[k] = -1;
        if (hipSetDevice(p->replicas[k]->device) != hipSuccess) {
            errs[k] = "hipSetDevice failed";
            return;
        }
        rc[k] = f(k);
        if (rc[k]) errs[k] = g_err;
    };
    if (n_gpus == 1) {
        run(0);
    } else {
        std::vector<std::thread> th;
        for (int k = 0; k < n_gpus; k++) th.emplace_back(run, k);
        for (auto &t : th) t.join();
    }
    for (int k = 0; k < n_gpus; k++)
        if (rc[k]) return fail("%s, device %d: %s", what, p->replicas[k]->device, errs[k].c_str());
    return 0;
}

// make_beam's reduce (src/solve.jl:233-240): d_dP[k] (n_psi + 1 fp64 on replica
// k's device) <- sum over k, in place on every replica (all-reduce semantics).
// RCCL over xGMI from a single-process communicator (ncclCommInitAll, kept on
// the handle) enqueued on the replicas' streams; the test-only same-device
// placement sums on the host.  Synchronous: the replicas' streams are drained.
static int beam_reduce_run(torj_plasma_s *p, int n_gpus, const std::vector<double *> &d_dP,
                           int n_psi, bool same);
static int beam_reduce(torj_plasma_s *p, int n_gpus, const std::vector<double *> &d_dP, int n_psi,
                       bool same) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = beam_reduce_run(p, n_gpus, d_dP, n_psi, same);
    if (p->timing && !rc) {
        p->reduce_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        p->reduce_calls++;
    }
    return rc;
}
static int beam_reduce_run(torj_plasma_s *p, int n_gpus, const std::vector<double *> &d_dP,
                           int n_psi, bool same) {
    const size_t m = (size_t)n_psi + 1;
    if (same) {
        std::vector<double> acc(m, 0.0), part(m);
        for (int k = 0; k < n_gpus; k++) {
            torj_plasma_s *q = p->replicas[k];
            HIPCK(hipSetDevice(q->device));
            HIPCK(hipMemcpyAsync(part.data(), d_dP[k], m * sizeof(double), hipMemcpyDeviceToHost, q->stream));
            HIPCK(hipStreamSynchronize(q->stream));
            for (size_t j = 0; j < m; j++) acc[j] += part[j];
        }
        for (int k = 0; k < n_gpus; k++) {
            torj_plasma_s *q = p->replicas[k];
            HIPCK(hipSetDevice(q->device));
            HIPCK(hipMemcpyAsync(d_dP[k], acc.data(), m * sizeof(double), hipMemcpyHostToDevice, q->stream));
            HIPCK(hipStreamSynchronize(q->stream));
        }
        return 0;
    }
    if ((int)p->comms.size() != n_gpus) {
        for (ncclComm_t c : p->comms) (void)ncclCommDestroy(c);
        p->comms.assign(n_gpus, nullptr);
        std::vector<int> devs(n_gpus);
        for (int k = 0; k < n_gpus; k++) devs[k] = p->replicas[k]->device;
        if (ncclCommInitAll(p->comms.data(), n_gpus, devs.data()) != ncclSuccess) {
            p->comms.clear();
            return fail("ncclCommInitAll over %d devices failed", n_gpus);
        }
    }
    ncclResult_t r = ncclGroupStart();
    for (int k = 0; k < n_gpus && r == ncclSuccess; k++)
        r = ncclAllReduce(d_dP[k], d_dP[k], m, ncclDouble, ncclSum, p->comms[k], p->replicas[k]->stream);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r != ncclSuccess || r2 != ncclSuccess)
        return fail("ncclAllReduce of dP_shell failed: %s", ncclGetErrorString(r != ncclSuccess ? r : r2));
    for (int k = 0; k < n_gpus; k++) {
        HIPCK(hipSetDevice(p->replicas[k]->device));
        HIPCK(hipStreamSynchronize(p->replicas[k]->stream));
    }
    return 0;
}

// Contiguous shard k of S over n rays, boundaries on 64-ray (one wave, one
// work-queue group) multiples, so every shard holds the same 64-ray groups as
// the unsplit beam and per-ray results do not depend on the split.
static void beam_shard(int n, int S, int k, int &lo, int &cnt) {
    const long G = (n + 63) / 64;
    const long g0 = G * k / S, g1 = G * (k + 1) / S;
    lo = (int)std::min<long>(g0 * 64, n);
    cnt = (int)std::min<long>(g1 * 64, n) - lo;
}

// The staging of torj_trace_beam on replica q: device and host memory for
// `nslots` (1 or 2) shard slots of `slot` doubles each, the copy stream and the
// events.  The host side is pinned while it fits TORJ_BEAM_PIN_MB (default
// 2048 MiB per replica; the transfers then run at PCIe rate and overlap the
// trace), pageable above it (hipMemcpyAsync stages those copies itself: slower,
// but a beam of huge user shards never fails for want of pinnable memory).
static int beam_stage(torj_plasma_s *q, size_t slot, int nslots) {
    auto &b = q->stage;
    if (!b.sc) {
        HIPCK(hipStreamCreateWithFlags(&b.sc, hipStreamNonBlocking));
        for (int r = 0; r < 2; r++) {
            HIPCK(hipEventCreateWithFlags(&b.up[r], hipEventDisableTiming));
            HIPCK(hipEventCreateWithFlags(&b.tr[r], hipEventDisableTiming));
            HIPCK(hipEventCreateWithFlags(&b.dn[r], hipEventDisableTiming));
        }
    }
    const size_t bytes = (size_t)nslots * slot * sizeof(double);
    if (b.d_cap < bytes) {
        if (b.d) HIPCK(hipFree(b.d));
        b.d = nullptr, b.d_cap = 0;
        HIPCK(hipMalloc(&b.d, bytes));
        b.d_cap = bytes;
    }
    const size_t pin_max = (size_t)env_long("TORJ_BEAM_PIN_MB", 2048) << 20;
    const bool pin = bytes <= pin_max;
    if (b.h_cap < bytes || (b.h_pinned && !pin)) {
        if (b.h) {
            if (b.h_pinned)
                HIPCK(hipHostFree(b.h));
            else
                free(b.h);
        }
        b.h = nullptr, b.h_cap = 0;
        if (pin) {
            HIPCK(hipHostMalloc(&b.h, bytes, hipHostMallocDefault));
        } else {
            b.h = malloc(bytes);
            if (!b.h) return fail("torj_trace_beam: host staging of %zu bytes failed", bytes);
        }
        b.h_cap = bytes;
        b.h_pinned = pin;
    }
    return 0;
}

// One device's share of torj_trace_beam: its shards k0, k0 + dk, ... traced on
// the replica's stream from compact device buffers, with dP_shell accumulated
// on the device (d_dP, zeroed here) for the reduce.  `host`'s arrays are the
// caller's (pageable); each shard goes through pinned staging in two slots on
// a copy stream, pipelined so that shard j + 1's upload and shard j - 1's
// download overlap shard j's trace:
//   copy stream  up(0) up(1) [tr 0] dn(0) up(2) [tr 1] dn(1) up(3) ...
//   trace stream        [up 0] trace(0) [up 1, dn of 2 shards back] trace(1) ...
// The host packs shard j + 1's inputs into its pinned slot while shard j
// traces, and unpacks shard j - 2's outputs (waiting for their download)
// before the slot's next download is queued.  A shard's rows are compact
// (row r of an array at r * cnt) on both sides, so each transfer is one copy;
// a slot's input and output blocks sit at fixed offsets (sized for the
// largest shard), so they never overlap across shards of different sizes.
static int beam_worker(torj_plasma_s *q, const torj_trace_cfg *cfg, const RayIO &host, int S, int k0, int dk,
                       int n_psi, double *d_dP) {
    if (ensure_device(q)) return -1;
    hipStream_t s = q->stream;
    const int n = host.n;
    const bool depo = n_psi >= 2 && host.psi_grid;
    const bool tr_out = host.traj && cfg->traj_stride > 0 && cfg->n_steps / cfg->traj_stride > 0;
    const int n_save = tr_out ? cfg->n_steps / cfg->traj_stride : 0;
    std::vector<int> los, cnts;  // this device's shards
    int m = 0;
    for (int k = k0; k < S; k += dk) {
        int lo, cnt;
        beam_shard(n, S, k, lo, cnt);
        if (cnt == 0) continue;
        los.push_back(lo), cnts.push_back(cnt);
        m = std::max(m, cnt);
    }
    if (depo) HIPCK(hipMemsetAsync(d_dP, 0, (n_psi + 1) * sizeof(double), s));
    if (m == 0) return 0;
    DevBufs B;
    double *dgrid = nullptr;
    if (depo && B.up(&dgrid, host.psi_grid, n_psi, s)) return -1;
    // rows per shard: inputs x0 N0 [w] [x_launch] [s0]; outputs state [P_dep]
    // [traj], then status and steps (two int rows in one double row)
    const int n_in = 6 + (host.weights ? 1 : 0) + (host.x_launch ? 3 : 0) + (host.s0 ? 1 : 0);
    const int n_out = 7 + (depo ? 1 : 0) + n_save * 5 + 1;
    const size_t slot = (size_t)(n_in + n_out) * m;
    const int nk = (int)los.size();
    if (beam_stage(q, slot, nk > 1 ? 2 : 1)) return -1;  // one shard: no second slot
    auto &bs = q->stage;
    double *dbase = (double *)bs.d, *hbase = (double *)bs.h;
    struct View {  // one slot's arrays for a shard of cnt rays
        double *x0, *N0, *w, *xl, *s0, *state, *Pdep, *traj;
        int *status, *steps;
        double *in, *out;  // the contiguous input / output blocks
        size_t n_in, n_out;  // their sizes in doubles
    };
    auto view = [&](double *base, int r, int cnt) {
        View v{};
        double *c = base + (size_t)r * slot;
        v.in = c;
        v.x0 = c, c += 3 * (size_t)cnt;
        v.N0 = c, c += 3 * (size_t)cnt;
        if (host.weights) v.w = c, c += cnt;
        if (host.x_launch) v.xl = c, c += 3 * (size_t)cnt;
        if (host.s0) v.s0 = c, c += cnt;
        v.n_in = c - v.in;
        // outputs at a fixed offset (m rays' inputs), so a shard's outputs never
        // share bytes with the next shards' inputs in the same slot: shard
        // j - 2's download into the host slot can land while shard j's inputs
        // are packed there
        c = v.in + (size_t)n_in * m;
        v.out = c;
        v.state = c, c += 7 * (size_t)cnt;
        if (depo) v.Pdep = c, c += cnt;
        if (n_save) v.traj = c, c += (size_t)n_save * 5 * cnt;
        v.status = (int *)c, v.steps = (int *)c + cnt, c += cnt;
        v.n_out = c - v.out;
        return v;
    };
    const size_t D = sizeof(double);
    // rows x cnt sub-block of a (rows x n) SoA host array <-> compact rows
    auto pack = [&](double *dst, const double *src, int rows, int lo, int cnt) {
        if (!src) return;
#pragma omp parallel for if ((size_t)rows * cnt > (1u << 18)) num_threads(8)
        for (int r = 0; r < rows; r++) memcpy(dst + (size_t)r * cnt, src + (size_t)r * n + lo, cnt * D);
    };
    auto unpack = [&](double *dst, const double *src, int rows, int lo, int cnt) {
        if (!dst) return;
#pragma omp parallel for if ((size_t)rows * cnt > (1u << 18)) num_threads(8)
        for (int r = 0; r < rows; r++) memcpy(dst + (size_t)r * n + lo, src + (size_t)r * cnt, cnt * D);
    };
    auto stage_in = [&](int j) -> int {  // pack shard j and queue its upload
        const int r = j & 1, lo = los[j], cnt = cnts[j];
        if (j >= 2) HIPCK(hipEventSynchronize(bs.up[r]));  // shard j - 2's upload left the slot
        const View h = view(hbase, r, cnt), d = view(dbase, r, cnt);
        pack(h.x0, host.x0, 3, lo, cnt), pack(h.N0, host.N0, 3, lo, cnt), pack(h.w, host.weights, 1, lo, cnt);
        pack(h.xl, host.x_launch, 3, lo, cnt), pack(h.s0, host.s0, 1, lo, cnt);
        HIPCK(hipMemcpyAsync(d.in, h.in, h.n_in * D, hipMemcpyHostToDevice, bs.sc));
        HIPCK(hipEventRecord(bs.up[r], bs.sc));
        return 0;
    };
    auto finish = [&](int j) -> int {  // wait for shard j's download, unpack it
        const int r = j & 1, lo = los[j], cnt = cnts[j];
        HIPCK(hipEventSynchronize(bs.dn[r]));
        const View h = view(hbase, r, cnt);
        unpack(host.state, h.state, 7, lo, cnt);
        if (depo) unpack(host.P_dep, h.Pdep, 1, lo, cnt);
        if (n_save) unpack(host.traj, h.traj, n_save * 5, lo, cnt);
        memcpy(host.status + lo, h.status, cnt * sizeof(int));
        memcpy(host.steps + lo, h.steps, cnt * sizeof(int));
        return 0;
    };
    // TORJ_BEAM_SYNC=1 (read per call; diagnosis): drain the device after every
    // queued step, so the pipeline runs in program order
    const bool dbg_sync = env_int("TORJ_BEAM_SYNC", 0) != 0;
    auto dsync = [&]() -> int {
        if (dbg_sync) HIPCK(hipDeviceSynchronize());
        return 0;
    };
    if (stage_in(0) || dsync()) return -1;
    for (int j = 0; j < nk; j++) {
        const int r = j & 1, cnt = cnts[j];
        if (j + 1 < nk && (stage_in(j + 1) || dsync())) return -1;
        const View d = view(dbase, r, cnt);
        HIPCK(hipStreamWaitEvent(s, bs.up[r], 0));
        if (j >= 2) HIPCK(hipStreamWaitEvent(s, bs.dn[r], 0));  // the slot's previous outputs are out
        RayIO io{};  // the shard on the device: its slot's arrays (Pdep only with deposition), no counters
        io.n = cnt, io.x0 = d.x0, io.N0 = d.N0, io.weights = d.w, io.x_launch = d.xl, io.s0 = d.s0;
        io.state = d.state, io.status = d.status, io.steps = d.steps, io.P_dep = d.Pdep, io.traj = d.traj;
        io.psi_grid = dgrid, io.dP_shell = depo ? d_dP : nullptr;
        if (trace_device(q, cfg, io, depo ? n_psi : 0, s)) return -1;
        HIPCK(hipEventRecord(bs.tr[r], s));
        if (dsync()) return -1;
        if (j >= 2 && finish(j - 2)) return -1;  // before this slot's host buffer is reused
        const View h = view(hbase, r, cnt);
        HIPCK(hipStreamWaitEvent(bs.sc, bs.tr[r], 0));
        HIPCK(hipMemcpyAsync(h.out, d.out, d.n_out * D, hipMemcpyDeviceToHost, bs.sc));
        HIPCK(hipEventRecord(bs.dn[r], bs.sc));
    }
    for (int j = std::max(0, nk - 2); j < nk; j++)
        if (finish(j)) return -1;
    // every shard's queue / grid flags (sticky since the last check)
    return torj_trace_check(q, s);
}

// Shards of torj_trace_beam when the caller leaves n_shards = 0: each device's
// share in pieces of at most kBeamAutoRays rays (at least one per device), so
// the host transfers of one piece overlap the trace of the next (beam_worker)
// while every piece still fills the device (the split pipeline wants >= ~1e5
// rays: a 1e5-ray beam stays one piece).
constexpr long kBeamAutoRays = 131072;
static int beam_auto_shards(int n, int n_gpus) {
    const long per = ((long)n + n_gpus - 1) / n_gpus;
    return n_gpus * (int)std::max<long>(1, (per + kBeamAutoRays - 1) / kBeamAutoRays);
}

