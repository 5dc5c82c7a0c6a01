// torj_fan.hpp -- host quadrature and the launch fan: Gauss-Legendre nodes
// (abs_Al_init), Gauss-Hermite nodes and the rings of peripheral rays.
// (a slice of torj_hip.hip / torj_traj.hip: included after `using namespace torj`)
#pragma once
#include <cmath>
#include <vector>

#include "torj_math.hpp"

static void gauss_legendre(int n, double *x, double *w) {
    const int m = (n + 1) / 2;
    for (int i = 0; i < m; i++) {
        double z = std::cos(kPi * (i + 0.75) / (n + 0.5)), pp = 1.0;
        for (int it = 0; it < 100; it++) {
            double p0 = 1.0, p1 = z;  // P_0, P_1
            for (int j = 2; j <= n; j++) {
                const double p2 = ((2.0 * j - 1.0) * z * p1 - (j - 1.0) * p0) / j;
                p0 = p1;
                p1 = p2;
            }
            if (n == 1) p0 = 1.0, p1 = z;
            pp = n * (z * p1 - p0) / (z * z - 1.0);
            const double dz = p1 / pp;
            z -= dz;
            if (std::fabs(dz) < 1e-16) break;
        }
        x[i] = -z;
        x[n - 1 - i] = z;
        w[i] = w[n - 1 - i] = 2.0 / ((1.0 - z * z) * pp * pp);
    }
}

// ===========================================================================
// launch fan (host), src/launch.jl:24-132
// ===========================================================================
// Orthonormal Hermite recurrence, rescaled by 2^-500 past 2^500 (overflow-free
// for any n); returns p_n, p_{n-1} and the binary exponent of the scale.
static void herm_rec(int n, double z, double &pn, double &pn1, int &e2) {
    double p1 = 0.7511255444649425, p2 = 0.0;  // pi^(-1/4)
    int e = 0;
    for (int j = 0; j < n; j++) {
        const double p3 = p2;
        p2 = p1;
        p1 = z * std::sqrt(2.0 / (j + 1)) * p2 - std::sqrt((double)j / (j + 1)) * p3;
        if (std::fabs(p1) > 0x1p500) {
            p1 = std::ldexp(p1, -500);
            p2 = std::ldexp(p2, -500);
            e += 500;
        }
    }
    pn = p1;
    pn1 = p2;
    e2 = e;
}

// FastGaussQuadrature.gausshermite(n) (src/launch.jl:72): ascending nodes,
// weight exp(-x^2).  Zeros are bracketed by sign changes on a grid finer than
// the smallest zero spacing (~pi/sqrt(2n+1), at the origin), bisected and
// Newton-polished -- robust for every n (asymptotic initial guesses are not).
static void gauss_hermite(int n, std::vector<double> &x, std::vector<double> &w) {
    std::vector<double> pos, pw;
    const int half = n / 2;
    const double zmax = std::sqrt(2.0 * n + 1.0) + 1.0;
    const double dz = 0.2 * kPi / std::sqrt(2.0 * n + 1.0);
    double a = (n & 1) ? 0.5 * dz : 0.0, fa, fa1;
    int ea;
    herm_rec(n, a, fa, fa1, ea);
    while ((int)pos.size() < half && a < zmax) {
        const double b = a + dz;
        double fb, fb1;
        int eb;
        herm_rec(n, b, fb, fb1, eb);
        if ((fa > 0) != (fb > 0) && fb != 0.0) {
            double lo = a, hi = b, flo = fa;
            for (int it = 0; it < 60; it++) {
                const double m = 0.5 * (lo + hi);
                double fm, fm1;
                int em;
                herm_rec(n, m, fm, fm1, em);
                if ((fm > 0) == (flo > 0)) {
                    lo = m;
                    flo = fm;
                } else {
                    hi = m;
                }
            }
            double z = 0.5 * (lo + hi), pn, pn1;
            int e;
            for (int it = 0; it < 3; it++) {
                herm_rec(n, z, pn, pn1, e);
                z -= pn / (std::sqrt(2.0 * n) * pn1);
            }
            herm_rec(n, z, pn, pn1, e);
            pos.push_back(z);
            pw.push_back(std::ldexp(1.0 / (n * pn1 * pn1), -2 * e));
        }
        a = b;
        fa = fb;
    }
    x.clear();
    w.clear();
    for (int i = (int)pos.size() - 1; i >= 0; i--) {
        x.push_back(-pos[i]);
        w.push_back(pw[i]);
    }
    if (n & 1) {
        double pn, pn1;
        int e;
        herm_rec(n, 0.0, pn, pn1, e);
        x.push_back(0.0);
        w.push_back(std::ldexp(1.0 / (n * pn1 * pn1), -2 * e));
    }
    for (size_t i = 0; i < pos.size(); i++) {
        x.push_back(pos[i]);
        w.push_back(pw[i]);
    }
}

struct Rings {
    std::vector<double> r, rw;
    std::vector<int> nth;
    int total = 0;
};

static Rings make_rings(int N_rings, int min_az, double w) {
    Rings R;
    std::vector<double> x, wt;
    gauss_hermite(2 * N_rings + 2, x, wt);  // :72
    for (int i = 0; i < N_rings; i++) {
        R.r.push_back(x[N_rings + 1 + i] * (w / std::sqrt(2.0)));
        R.rw.push_back(wt[N_rings + 1 + i] * (w / std::sqrt(2.0)));
    }
    for (int i = 0; i < N_rings; i++) {  // :80-83, Julia's round(Int64, x): ties to even
        const long k = round_ties_even(min_az * R.r[i] / R.r[0]);
        R.nth.push_back(k < 1 ? 1 : (int)k);
        R.total += R.nth.back();
    }
    return R;
}

