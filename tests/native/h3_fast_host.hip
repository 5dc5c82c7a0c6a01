// Host build of abs_Albajar_fast (torj.jl_amd/csrc/torj_math.hpp is __host__
// __device__) around harmonic 3's dismissal from the prologue's outputs
// (h3_fast_negligible): per point, alpha with GLTable::h3_fast on and off, the
// test's verdict and bounds, and what albajar_harmonic<3> itself does there.
// Test harness only (tests/test_h3_fast_host.py).
#include "torj_math.hpp"

#include <cmath>

static torj::GLTable g_gl;

extern "C" {
// the Gauss-Legendre table as torj_abs_al_init makes it (ascending nodes, zero-padded)
void hf_setup(int ngl, const double *t, const double *w) {
    g_gl = torj::GLTable{};
    g_gl.n = ngl;
    g_gl.negl_skip = 1;
    for (int i = 0; i < torj::kMaxGL; i++) {
        g_gl.t[i] = i < ngl ? t[i] : 0.0;
        g_gl.w[i] = i < ngl ? w[i] : 0.0;
        g_gl.st[i] = i < ngl ? sqrt(1.0 - t[i] * t[i]) : 0.0;
        g_gl.t2[i] = i < ngl ? t[i] * t[i] : 0.0;
        if (i < ngl) torj::gl_node_consts(g_gl, i);
    }
}

// n points, tiny = GLTable::tiny_alpha.  Outputs per point:
//  alpha_on / alpha_off: abs_albajar_fast_body with h3_fast 1 / 0;
//  reach: 1 where Te >= 20, harmonic 3 is present and the prologue is ok (the
//         points at which abs_albajar_fast_body can evaluate the test; those it
//         settles before the polarisation vector are kept: a wider check);
//  verdict: h3_fast_negligible; bound: U 2^(ceil(y_ub) + 1); y_ub (inf, inf where
//         h3_fast_bound refuses);
//  b0e, ymax: albajar_harmonic<3>'s B0 E_max and harm_geom(3)'s ymax;
//  outcome: albajar_harmonic<3> there: 0 integrated, 1 exact zero, 2 skipped as negligible
void hf_eval(int n, const double *om, const double *X, const double *Y, const double *Nabs,
             const double *Npar, const double *Te, int mode, double tiny, double *alpha_on,
             double *alpha_off, int *reach, int *verdict, double *bound, double *y_ub, double *b0e,
             double *ymax, int *outcome) {
    using namespace torj;
    for (int i = 0; i < n; i++) {
        g_gl.tiny_alpha = tiny;
        g_gl.h3_fast = 1;
        alpha_on[i] = abs_albajar_fast_body<1>(g_gl, om[i], X[i], Y[i], Nabs[i], Npar[i], Te[i], mode,
                                               nullptr, 0, tiny);
        g_gl.h3_fast = 0;
        alpha_off[i] = abs_albajar_fast_body<1>(g_gl, om[i], X[i], Y[i], Nabs[i], Npar[i], Te[i], mode,
                                                nullptr, 0, tiny);
        reach[i] = verdict[i] = 0;
        outcome[i] = -1;
        bound[i] = y_ub[i] = b0e[i] = ymax[i] = NAN;
        if (Te[i] < 20.0) continue;
        const AlbPre pre = albajar_pre(Y[i], Nabs[i], Npar[i], Te[i]);
        const bool h2 = !(2.0 < pre.m_0), h3 = !(3.0 < pre.m_0);
        if (!h3) continue;
        const AlbPro q = albajar_prologue(pre, X[i], Y[i], Nabs[i], Npar[i], mode);
        if (!q.ok) continue;
        reach[i] = 1;
        const double hmax = tiny_harmonic(tiny, q, X[i], om[i]);
        double dom = 0.0;
        if (h2) {
            const HarmGeom g2 = harm_geom(pre.mu, pre.inv_mu, 2.0 * pre.inv_m0, Npar[i], pre.inv_sqNp);
            dom += albajar_pro_harmonic<2, 1>(g_gl, q, g2, nullptr, 0, 0.0, hmax);
        }
        verdict[i] = h3_fast_negligible(pre, q, Npar[i], hmax, dom) ? 1 : 0;
        double U, yu;
        if (!h3_fast_bound(pre, q, Npar[i], U, yu)) U = yu = INFINITY;
        y_ub[i] = yu;
        bound[i] = U * h3_fast_emax(yu);
        // the present path's own quantities
        const HarmGeom g3 = harm_geom(pre.mu, pre.inv_mu, 3.0 * pre.inv_m0, Npar[i], pre.inv_sqNp);
        ymax[i] = g3.ymax;
        const HarmConst c = harm_consts<3>(q.mu, g3, q.inv_sqNp, q.N_perp, q.omega_bar, q.Axz, q.ea, q.e3);
        const double den = q.N_perp * q.omega_bar;
        const double Pm = den == 0.0 ? INFINITY : 3.0 * rcp_nz(den);
        b0e[i] = harm_b0<3>(c, q.mu, Pm, g3.sq_r) * harm_emax(g3, c, q.mu);
        AlbajarWork wk{};
        (void)albajar_harmonic<3, 1>(g_gl, q.mu, g3, q.inv_sqNp, q.N_perp, q.omega_bar, q.Axz, q.ea, q.e3,
                                     &wk, 0, dom, hmax);
        outcome[i] = wk.n_zero ? 1 : (wk.n_negl ? 2 : 0);
    }
}
}
