// torj_coefbuild.hpp -- a plasma's node coefficients (d_coef, kNF doubles per node)
// built on the device from its node data: cb_prefilter_line, one line of
// bspl1d_prefilter, cb_prof_node, one node of make_2d_prof_spline, and the three
// kernels torj_plasma_update_gpu / _profiles_gpu / _device enqueue ahead of
// k_cell_table.
// (a slice of torj_hip.hip: included after `using namespace torj`; the host
// build of the two functions is tests/native/coefbuild_host.hip)
#pragma once
#include "torj_math.hpp"

// ---------------------------------------------------------------------------
// The host's prefilters (torj_plasma.hpp bspl1d_prefilter, bspl1d_eval) are
// IEEE + - * /, floor and compares in a fixed order.  The functions below are
// the same sequences, with contraction and reassociation off in every body and
// no helper compiled without that pragma (bweights is contracted on the
// device: its four weights are written out here), so the device build gives
// the host's bits.
// ---------------------------------------------------------------------------

// slot of field f (torj_plasma_get_coefs' order: psi, ln ne, ln Te, Br, Bz, Bphi)
// in a node's kNF doubles: torj_plasma.hpp kFieldSlot, one nibble per field
TORJ_HD int cb_field_slot(int f) { return (0x120435 >> (4 * f)) & 15; }

// The Thomas sweep's pivots, which depend on the row index alone:
// cp[k] = 1 / (4 - cp[k - 1]), bspl1d_prefilter's `cp`, for k < m.  One table
// serves every line of a plasma (m = max(nR, nZ) - 2).
TORJ_HD void cb_pivots(int m, double *cp) {
#pragma clang fp contract(off) reassociate(off)
    for (int k = 0; k < m; k++) {
        const double den = 4.0 - (k > 0 ? cp[k - 1] : 0.0);
        cp[k] = 1.0 / den;
    }
}

// One line of bspl1d_prefilter: n values y (stride ys) -> n + 2 coefficients c
// (stride cs), cp the pivots above (n - 2 or more).  The forward sweep's dp[k]
// lives in c[k + 2].  y may be c + cs with ys == cs, the line prefiltered in
// place (y[k] is c[k + 1]): every value is read before its place is written.
TORJ_HD void cb_prefilter_line(int n, const double *y, size_t ys, double *c, size_t cs, const double *cp) {
#pragma clang fp contract(off) reassociate(off)
    const double c1 = y[0], cn = y[(size_t)(n - 1) * ys];
    c[cs] = c1;
    c[(size_t)n * cs] = cn;
    const int m = n - 2;  // interior unknowns c_2..c_{n-1}
    if (m > 0) {
        double dprev = 0.0;
        for (int k = 0; k < m; k++) {
            double r = 6.0 * y[(size_t)(k + 1) * ys];
            if (k == 0) r -= c1;
            if (k == m - 1) r -= cn;
            const double den = 4.0 - (k > 0 ? cp[k - 1] : 0.0);
            dprev = (r - dprev) / den;
            c[(size_t)(k + 2) * cs] = dprev;
        }
        double cnext = dprev;  // c[m + 1] = dp[m - 1]
        for (int k = m - 2; k >= 0; k--) {
            cnext = c[(size_t)(k + 2) * cs] - cp[k] * cnext;
            c[(size_t)(k + 2) * cs] = cnext;
        }
    }
    c[0] = 2.0 * c[cs] - c[2 * cs];
    c[(size_t)(n + 1) * cs] = 2.0 * c[(size_t)n * cs] - c[(size_t)(n - 1) * cs];
}

// One node of make_2d_prof_spline: bspl1d_eval of the 1-D ln-profile
// coefficients c1 (n + 2 over the uniform range [x1, xn]) at the node's psi,
// the clamp and the Line() slope term outside the range included.
TORJ_HD double cb_prof_node(const double *c1, int n, double x1, double xn, double x) {
#pragma clang fp contract(off) reassociate(off)
    const double h = (xn - x1) / (double)(n - 1);
    const double xc = x > xn ? xn : (x < x1 ? x1 : x);
    const double u = (xc - x1) / h;
    int i = (int)floor(u);
    i = i > n - 2 ? n - 2 : i;
    i = i < 0 ? 0 : i;
    // bweights(u - i, w, dw)
    const double d = u - (double)i;
    const double p = 1.0 - d;
    const double d2 = d * d, p2 = p * p;
    const double w0 = p2 * p * (1.0 / 6.0);
    const double w1 = 2.0 / 3.0 - d2 + 0.5 * d2 * d;
    const double w2 = 2.0 / 3.0 - p2 + 0.5 * p2 * p;
    const double w3 = d2 * d * (1.0 / 6.0);
    const double dw0 = -0.5 * p2;
    const double dw1 = -2.0 * d + 1.5 * d2;
    const double dw2 = 2.0 * p - 1.5 * p2;
    const double dw3 = 0.5 * d2;
    const double c0 = c1[i], ca = c1[i + 1], cb = c1[i + 2], cc = c1[i + 3];
    double v = 0.0, g = 0.0;
    v = v + w0 * c0;
    g = g + dw0 * c0;
    v = v + w1 * ca;
    g = g + dw1 * ca;
    v = v + w2 * cb;
    g = g + dw2 * cb;
    v = v + w3 * cc;
    g = g + dw3 * cc;
    return v + (x - xc) * (g / h);
}

// What the three kernels take.  Fields f0 .. f0 + nf - 1 of cb_field_slot's order
// are built: all six (f0 = 0, nf = 6), or ln ne and ln Te alone (f0 = 1, nf = 2).
struct CoefBuild {
    double *coef;                          // d_coef: (nR + 2) x (nZ + 2) nodes, kNF doubles each
    const double *psi, *Br, *Bz, *Bphi;    // node maps, nR x nZ, R fastest (Br, Bz, Bphi unused at nf = 2)
    const double *c1_ne, *c1_te;           // 1-D ln-profile coefficients, n_prof + 2 each
    const double *cp;                      // cb_pivots, max(nR, nZ) - 2
    double x1, xn;                         // the profiles' psi range
    int n_prof, nR, nZ, f0, nf;
};

// (TORJ_COEFBUILD_NO_KERNEL: a host-only build of the functions above, which has
// no device code object for a kernel to live in)
#ifndef TORJ_COEFBUILD_NO_KERNEL
// Node values into their own nodes' slots, coef[(j + 1, i + 1)], where the
// in-place passes below read them: one thread per (node, field), field fastest,
// so a wave writes the built slots of consecutive nodes.
__global__ __launch_bounds__(256) void k_coef_nodes(CoefBuild a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long)a.nR * a.nZ * a.nf) return;
    const long node = t / a.nf;
    const int f = a.f0 + (int)(t - node * a.nf);
    const int j = (int)(node / a.nR), i = (int)(node - (long)j * a.nR);
    double v;
    if (f == 1 || f == 2) {
        v = cb_prof_node(f == 1 ? a.c1_ne : a.c1_te, a.n_prof, a.x1, a.xn, a.psi[node]);
    } else {
        const double *m = f == 0 ? a.psi : (f == 3 ? a.Br : (f == 4 ? a.Bz : a.Bphi));
        v = m[node];
    }
    a.coef[((size_t)(j + 1) * (a.nR + 2) + (size_t)(i + 1)) * kNF + cb_field_slot(f)] = v;
}

// One thread per (line, field), field fastest, each line prefiltered in place.
// along_Z false: the nZ rows of node values along R (a wave's lanes: the built
// slots of one node, then the next row's).  along_Z true: the nR + 2 columns
// along Z (a wave's lanes: the built slots of consecutive nodes of a row).
__global__ __launch_bounds__(64) void k_coef_prefilter(CoefBuild a, bool along_Z) {
    const int lines = along_Z ? a.nR + 2 : a.nZ;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lines * a.nf) return;
    const int line = t / a.nf;
    const int f = a.f0 + (t - line * a.nf);
    const size_t mR = (size_t)a.nR + 2;
    if (along_Z) {
        double *c = a.coef + (size_t)line * kNF + cb_field_slot(f);
        cb_prefilter_line(a.nZ, c + mR * kNF, mR * kNF, c, mR * kNF, a.cp);
    } else {
        double *c = a.coef + (size_t)(line + 1) * mR * kNF + cb_field_slot(f);
        cb_prefilter_line(a.nR, c + kNF, kNF, c, kNF, a.cp);
    }
}
#endif
