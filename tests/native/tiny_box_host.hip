// Host build of the block tiny box (torj_math.hpp TBox, tiny_box_add,
// tiny_box_flag) beside the block zero box and abs_albajar_fast_body, which the
// disjunction of the two flags must never contradict: the trajectory kernel
// writes "zero_box_flag or tiny_box_flag" per ray and block, and its dead-box
// latch tests the same disjunction.  The stage point (ln Te, Y, N_par, |N|^2, X)
// reaches alpha as k_alpha_pts hands it on: |N| = sqrt_pos(|N|^2), Te =
// exp_fast(ln Te).
// Test harness only (tests/test_tiny_box_host.py).
#include "torj_math.hpp"

#include <cmath>
#include <vector>

static torj::GLTable g_gl;

namespace {
struct Boxes {
    torj::ZBox zb;
    torj::TBox tb;
};
inline void add(Boxes &b, const double *lnTe, const double *Y, const double *Npar, const double *N2,
                const double *X, size_t i) {
    // cold_step's order
    torj::zero_box_add(b.zb, lnTe[i], Y[i], Npar[i], N2[i]);
    torj::tiny_box_add(b.zb, b.tb, X[i], N2[i]);
}
inline bool either(const Boxes &b, double omega, int mode, double tiny) {
    return torj::zero_box_flag(b.zb) || torj::tiny_box_flag(b.zb, b.tb, omega, mode, tiny);
}
}  // namespace

extern "C" {
int tb_gamma_lin() { return TORJ_NODE_GAMMA_LIN; }

// the Gauss-Legendre table as torj_abs_al_init makes it (ascending nodes, zero-padded)
void tb_setup(int ngl, const double *t, const double *w) {
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

// nb boxes of k points each (point p of box b at b * k + p), added in order:
// zflag[b] = zero_box_flag, tflag[b] = tiny_box_flag
void tb_flags(int nb, int k, const double *lnTe, const double *Y, const double *Npar, const double *N2,
              const double *X, double omega, int mode, double tiny, int *zflag, int *tflag) {
    for (int b = 0; b < nb; b++) {
        Boxes bx;
        for (int p = 0; p < k; p++) add(bx, lnTe, Y, Npar, N2, X, (size_t)b * k + p);
        zflag[b] = torj::zero_box_flag(bx.zb) ? 1 : 0;
        tflag[b] = torj::tiny_box_flag(bx.zb, bx.tb, omega, mode, tiny) ? 1 : 0;
    }
}

// alpha at n stage points with GLTable::negl_skip, h3_fast and tiny_alpha as given
void tb_alpha(int n, const double *lnTe, const double *Y, const double *Npar, const double *N2,
              const double *X, double omega, int mode, int negl_skip, int h3_fast, double tiny, double *alpha) {
    using namespace torj;
    g_gl.negl_skip = negl_skip;
    g_gl.h3_fast = h3_fast;
    g_gl.tiny_alpha = tiny;
    for (int i = 0; i < n; i++)
        alpha[i] = abs_albajar_fast_body<1>(g_gl, omega, X[i], Y[i], sqrt_pos(N2[i]), Npar[i],
                                            exp_fast<true>(lnTe[i]), mode, nullptr, 0, tiny);
}

// zl_prefix of tests/native/zbox_latch_host.hip over the disjunction of the two
// flags; tiny_seen[b] = 1 when a prefix's flag was true by tiny_box_flag alone
void tb_prefix(int nb, int k, const double *lnTe, const double *Y, const double *Npar, const double *N2,
               const double *X, double omega, int mode, double tiny, int *final_flag, int *first_false,
               int *back, int *tiny_seen) {
    for (int b = 0; b < nb; b++) {
        Boxes bx;
        int ff = 0, bk = 0, ts = 0;
        bool f = true;
        for (int p = 0; p < k; p++) {
            add(bx, lnTe, Y, Npar, N2, X, (size_t)b * k + p);
            f = either(bx, omega, mode, tiny);
            if (f && !torj::zero_box_flag(bx.zb)) ts = 1;
            if (!f && !ff) ff = p + 1;
            if (f && ff && !bk) bk = p + 1;
        }
        final_flag[b] = f ? 1 : 0;
        first_false[b] = ff;
        back[b] = bk;
        tiny_seen[b] = ts;
    }
}

// zl_latched of tests/native/zbox_latch_host.hip with both boxes: traj_run's
// bookkeeping over `wave` lanes, the vote over the disjunction, the kill
// through the zero box's chk word, which both flags read
void tb_latched(int nb, int k, int stride, int wave, int ncad, const int *cad, const int *len,
                const double *lnTe, const double *Y, const double *Npar, const double *N2, const double *X,
                double omega, int mode, double tiny, int *flag, int *latched) {
    const int trips_max = k / stride;
    for (int w0 = 0; w0 < nb; w0 += wave) {
        const int nl = nb - w0 < wave ? nb - w0 : wave;
        std::vector<Boxes> bx(nl);
        bool zon = true;
        for (int l = 0; l < nl; l++) latched[w0 + l] = 0;
        for (int t = 0; t < trips_max; t++) {
            bool any_in = false;
            for (int l = 0; l < nl; l++) {
                if (t >= len[w0 + l]) continue;  // this lane has left the loop
                any_in = true;
                if (!zon) continue;
                for (int s = 0; s < stride; s++)
                    add(bx[l], lnTe, Y, Npar, N2, X, (size_t)(w0 + l) * k + (size_t)t * stride + s);
            }
            if (!any_in) break;
            bool due = false;
            for (int c = 0; c < ncad; c++) due = due || cad[c] == t + 1;
            if (!zon || !due) continue;
            bool any = false, voters = false;
            for (int l = 0; l < nl; l++)
                if (t + 1 < len[w0 + l] || (t + 1 == len[w0 + l] && t + 1 == trips_max)) {
                    voters = true;
                    any = any || either(bx[l], omega, mode, tiny);
                }
            if (voters && !any) {
                for (int l = 0; l < nl; l++)
                    if (t + 1 < len[w0 + l] || (t + 1 == len[w0 + l] && t + 1 == trips_max)) {
                        torj::zero_box_kill(bx[l].zb);
                        latched[w0 + l] = t + 1;
                    }
                zon = false;
            }
        }
        for (int l = 0; l < nl; l++) flag[w0 + l] = either(bx[l], omega, mode, tiny) ? 1 : 0;
    }
}
}
