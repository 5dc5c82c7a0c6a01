// Host build of the planning of a multi-beam launch through several plasmas
// (torj.jl_amd/csrc/torj_launch.hpp with TORJ_LAUNCH_PLAN_ONLY: no kernel, no HIP
// call): beams_plasmas_plan's argument checks, its per-beam plasma index, its plasma
// records and, beside it, beams_plan's wave table for the same beams.  The listed
// plasmas are stand-ins of this harness, read through a PlasmaView as the library
// reads its handles.  Test harness only (tests/test_beams_plasmas_plan.py).
#include <hip/hip_runtime.h>

#include "torj_math.hpp"

using namespace torj;

#define TORJ_LAUNCH_PLAN_ONLY 1
#include "torj_launch.hpp"

// a listed plasma as the test describes it: its device, and what its record must carry
struct FakePlasma {
    int device;
    PlasmaRec rec;
};
static const PlasmaView kFakeView = {[](const void *h) { return ((const FakePlasma *)h)->device; },
                                     [](const void *h) { return ((const FakePlasma *)h)->rec; }};

extern "C" {
// plasmas: n_plasmas x 6 doubles (device, coef tag, cellp tag, nR, nZ, psi_max), a negative
// device meaning a NULL entry; n_plasmas_arg is what the plan is told (the table may be NULL).
// has and knobs as beams_plan_host.hip's bp_plan.
// out: lanes per ray, waves, rays; beam_pl (n_beams); recs: per listed plasma (coef tag, cellp
// tag, nR, nZ, psi_max); waves (beam, first ray) of this plan and of beams_plan alone
int bpp_plan(const torj_trace_cfg *cfg, int n_plasmas_arg, int n_listed, const double *plasmas, int null_list,
             const int *beam_plasma, int device, int n_beams, const int *beam_off, const double *omega,
             const int *mode, int n_psi, int has, const int *knobs, long long *out, int *beam_pl, double *recs,
             int *waves, int *waves_ref, int waves_cap) {
    const LaunchPtrs hp = {(has & 1) != 0, (has & 2) != 0, (has & 4) != 0, (has & 8) != 0, (has & 16) != 0, (has & 32) != 0};
    const LaunchKnobs kn = {knobs[0], knobs[1], knobs[2], knobs[3], knobs[4], knobs[5], knobs[6], knobs[7], knobs[8]};
    std::vector<FakePlasma> fake(n_listed);
    std::vector<const void *> list(n_listed);
    for (int j = 0; j < n_listed; j++) {
        const double *q = plasmas + 6 * j;
        fake[j].device = (int)q[0];
        fake[j].rec = PlasmaRec{(const double *)(uintptr_t)q[1], (const double *)(uintptr_t)q[2], Grid{}, q[5]};
        fake[j].rec.g.nR = (int)q[3], fake[j].rec.g.nZ = (int)q[4];
        list[j] = q[0] < 0 ? nullptr : &fake[j];
    }
    BeamsPlasmasPlan pp;
    if (beams_plasmas_plan(pp, *cfg, n_plasmas_arg, null_list ? nullptr : list.data(), beam_plasma, device, kFakeView,
                           n_beams, beam_off, omega, mode, n_psi, hp, kn))
        return -1;
    BeamsPlan ref;
    if (beams_plan(ref, *cfg, n_beams, beam_off, omega, mode, n_psi, hp, kn)) return -2;
    out[0] = pp.bp.lpr, out[1] = (long long)pp.bp.waves.size(), out[2] = pp.bp.n;
    out[3] = (long long)ref.waves.size(), out[4] = ref.lpr, out[5] = (long long)pp.plasmas.size();
    out[6] = (long long)pp.beam_pl.size();
    for (size_t b = 0; b < pp.beam_pl.size(); b++) beam_pl[b] = pp.beam_pl[b];
    for (size_t j = 0; j < pp.plasmas.size(); j++) {
        const PlasmaRec &r = pp.plasmas[j];
        double *o = recs + 5 * j;
        o[0] = (double)(uintptr_t)r.coef, o[1] = (double)(uintptr_t)r.cellp, o[2] = r.g.nR, o[3] = r.g.nZ, o[4] = r.psi_max;
    }
    for (size_t w = 0; w < pp.bp.waves.size() && (int)w < waves_cap; w++)
        waves[2 * w] = pp.bp.waves[w].beam, waves[2 * w + 1] = pp.bp.waves[w].first;
    for (size_t w = 0; w < ref.waves.size() && (int)w < waves_cap; w++)
        waves_ref[2 * w] = ref.waves[w].beam, waves_ref[2 * w + 1] = ref.waves[w].first;
    return 0;
}
const char *bpp_error(void) { return g_err.c_str(); }
int bpp_max_plasmas(void) { return kMaxPlasmas; }
}
