// Host build of torj_coefbuild.hpp's cb_pivots, cb_prefilter_line and cb_prof_node (the
// functions k_coef_nodes and k_coef_prefilter run per lane on the device), looped over a
// whole plasma as those kernels' lanes do, for tests/test_coefbuild_host.py.  The 1-D
// parts are the library's own host functions (torj_plasma.hpp), as in
// torj_plasma_update_gpu.  Compiled with --offload-host-only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/torj_hip.h"
#include "torj_math.hpp"

using namespace torj;

#include "torj_plasma.hpp"
#define TORJ_COEFBUILD_NO_KERNEL 1
#include "torj_coefbuild.hpp"

extern "C" {

int cb_nf(void) { return kNF; }

// cb_field_slot against the host's table
int cb_slots_ok(void) {
    for (int f = 0; f < 6; f++)
        if (cb_field_slot(f) != kFieldSlot[f]) return 0;
    return 1;
}

// The interleaved coefficients, (nR + 2) x (nZ + 2) nodes of kNF doubles (zeroed first), of fields
// f0 .. f0 + nf - 1: k_coef_nodes' loop, then k_coef_prefilter's along R and along Z, each line
// in place.  Maps: nR x nZ, R fastest.
void cb_build(int nR, int nZ, const double *psi, const double *Br, const double *Bz, const double *Bphi, int n_prof,
              const double *psi_prof, const double *ne_prof, const double *Te_prof, int f0, int nf, double *coef) {
    const size_t mR = (size_t)nR + 2;
    std::vector<double> c1_ne, c1_te, cp((size_t)std::max(nR, nZ));
    prof1d_coefs(n_prof, psi_prof, ne_prof, c1_ne);
    prof1d_coefs(n_prof, psi_prof, Te_prof, c1_te);
    cb_pivots(std::max(nR, nZ) - 2, cp.data());
    const double x1 = psi_prof[0], xn = psi_prof[n_prof - 1];
    for (long t = 0; t < (long)nR * nZ * nf; t++) {
        const long node = t / nf;
        const int f = f0 + (int)(t - node * nf);
        const int j = (int)(node / nR), i = (int)(node - (long)j * nR);
        double v;
        if (f == 1 || f == 2) {
            v = cb_prof_node(f == 1 ? c1_ne.data() : c1_te.data(), n_prof, x1, xn, psi[node]);
        } else {
            const double *m = f == 0 ? psi : (f == 3 ? Br : (f == 4 ? Bz : Bphi));
            v = m[node];
        }
        coef[((size_t)(j + 1) * mR + (size_t)(i + 1)) * kNF + cb_field_slot(f)] = v;
    }
    for (int t = 0; t < nZ * nf; t++) {
        const int line = t / nf, f = f0 + (t - line * nf);
        double *c = coef + (size_t)(line + 1) * mR * kNF + cb_field_slot(f);
        cb_prefilter_line(nR, c + kNF, kNF, c, kNF, cp.data());
    }
    for (int t = 0; t < (nR + 2) * nf; t++) {
        const int line = t / nf, f = f0 + (t - line * nf);
        double *c = coef + (size_t)line * kNF + cb_field_slot(f);
        cb_prefilter_line(nZ, c + mR * kNF, mR * kNF, c, mR * kNF, cp.data());
    }
}

// cb_prefilter_line out of place against the host's bspl1d_prefilter on one line: 0 when every bit agrees
int cb_line_differs(int n, const double *y) {
    std::vector<double> a((size_t)n + 2, -1.0), b((size_t)n + 2, -2.0), cp((size_t)n);
    bspl1d_prefilter(n, y, 1, a.data(), 1);
    cb_pivots(n - 2, cp.data());
    cb_prefilter_line(n, y, 1, b.data(), 1, cp.data());
    int bad = 0;
    for (int k = 0; k < n + 2; k++) bad += __builtin_memcmp(&a[k], &b[k], sizeof(double)) != 0;
    return bad;
}

}  // extern "C"
