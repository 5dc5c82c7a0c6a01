// Host build of the split pipeline's block zero box (torj_math.hpp ZBox,
// zero_box_add, zero_box_flag) beside abs_albajar_fast_body, which it must
// never contradict, and of the tiny-alpha skip at single points.  The stage
// point (ln Te, Y, N_par, |N|^2, X) reaches alpha as k_alpha_pts hands it on:
// |N| = sqrt_pos(|N|^2), Te = exp_fast(ln Te).
// Test harness only (tests/test_skip_proofs_host.py).
#include "torj_math.hpp"

#include <cmath>

static torj::GLTable g_gl;

extern "C" {
int sp_gamma_lin() { return TORJ_NODE_GAMMA_LIN; }

// the Gauss-Legendre table as torj_abs_al_init makes it (ascending nodes, zero-padded)
void sp_setup(int ngl, const double *t, const double *w) {
    g_gl = torj::GLTable{};
    g_gl.n = ngl;
    g_gl.negl_skip = 1;
    g_gl.h3_fast = 1;
    for (int i = 0; i < torj::kMaxGL; i++) {
        g_gl.t[i] = i < ngl ? t[i] : 0.0;
        g_gl.w[i] = i < ngl ? w[i] : 0.0;
        g_gl.st[i] = i < ngl ? sqrt(1.0 - t[i] * t[i]) : 0.0;
        g_gl.t2[i] = i < ngl ? t[i] * t[i] : 0.0;
        if (i < ngl) torj::gl_node_consts(g_gl, i);
    }
}

// nb boxes of k points each (point p of box b at b * k + p), added in order as
// cold_step adds a block's stage points: flag[b] = zero_box_flag
void sp_flags(int nb, int k, const double *lnTe, const double *Y, const double *Npar, const double *N2,
              int *flag) {
    for (int b = 0; b < nb; b++) {
        torj::ZBox zb;
        for (int p = 0; p < k; p++) {
            const size_t i = (size_t)b * k + p;
            torj::zero_box_add(zb, lnTe[i], Y[i], Npar[i], N2[i]);
        }
        flag[b] = torj::zero_box_flag(zb) ? 1 : 0;
    }
}

// alpha at n stage points with GLTable::negl_skip and tiny_alpha as given
// (h3_fast follows negl_skip, as abs_Al_init sets them by default)
void sp_alpha(int n, const double *lnTe, const double *Y, const double *Npar, const double *N2,
              const double *X, double omega, int mode, int negl_skip, double tiny, double *alpha) {
    using namespace torj;
    g_gl.negl_skip = negl_skip;
    g_gl.h3_fast = negl_skip;
    g_gl.tiny_alpha = tiny;
    for (int i = 0; i < n; i++)
        alpha[i] = abs_albajar_fast_body<1>(g_gl, omega, X[i], Y[i], sqrt_pos(N2[i]), Npar[i],
                                            exp_fast<true>(lnTe[i]), mode, nullptr, 0, tiny);
}

// alpha at n points (X, Y, |N|, N_par, Te) as tests/test_h3_fast_host.py lays them out
void sp_alpha_pts(int n, const double *X, const double *Y, const double *Nabs, const double *Npar,
                  const double *Te, double omega, int mode, double tiny, double *alpha) {
    using namespace torj;
    g_gl.negl_skip = 1;
    g_gl.h3_fast = 1;
    g_gl.tiny_alpha = tiny;
    for (int i = 0; i < n; i++)
        alpha[i] = abs_albajar_fast_body<1>(g_gl, omega, X[i], Y[i], Nabs[i], Npar[i], Te[i], mode,
                                            nullptr, 0, tiny);
}
}
