// torj_celltab.hpp -- the per-cell power table (torj_math.hpp cell_power_table's
// layout) rebuilt on the device from the node coefficients: cell_record, one
// (cell, field) record in double-double arithmetic, and k_cell_table, the
// kernel torj_plasma_update[_from_coefs, _profiles] enqueues behind the copy of
// the new coefficients.
// (a slice of torj_hip.hip: included after `using namespace torj`; the host
// build of cell_record is tests/native/cell_table_host.hip)
#pragma once
#include "torj_math.hpp"

// ---------------------------------------------------------------------------
// double-double: an unevaluated sum hi + lo with |lo| <= ulp(hi) / 2.  The
// device has no long double; two-sum and the fma two-product are exact, so the
// host and the device build of the functions below give the same bits as long
// as the compiler neither contracts nor reassociates them: every fma is
// explicit, and each body turns contraction and reassociation off.
// ---------------------------------------------------------------------------
struct DD {
    double hi, lo;
};
// a + b exactly (Knuth), any magnitudes
TORJ_HD DD dd_two_sum(double a, double b) {
#pragma clang fp contract(off) reassociate(off)
    const double s = a + b;
    const double bb = s - a;
    const double e = (a - (s - bb)) + (b - bb);
    return {s, e};
}
// a + b exactly for |a| >= |b| (or a == 0)
TORJ_HD DD dd_fast_two_sum(double a, double b) {
#pragma clang fp contract(off) reassociate(off)
    const double s = a + b;
    const double e = b - (s - a);
    return {s, e};
}
// a * b exactly
TORJ_HD DD dd_two_prod(double a, double b) {
#pragma clang fp contract(off) reassociate(off)
    const double p = a * b;
    const double e = __builtin_fma(a, b, -p);
    return {p, e};
}
// x + y, relative error <= 3 * 2^-106 whatever the cancellation (the
// "accurate" sum: both halves by two-sum)
TORJ_HD DD dd_add(DD x, DD y) {
#pragma clang fp contract(off) reassociate(off)
    DD s = dd_two_sum(x.hi, y.hi);
    const DD t = dd_two_sum(x.lo, y.lo);
    s.lo = s.lo + t.hi;
    s = dd_fast_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return dd_fast_two_sum(s.hi, s.lo);
}
// x / d for a double d: three quotient digits (each a correctly rounded double
// division, the same on host and device), the remainders taken exactly;
// relative error below 2^-100
TORJ_HD DD dd_div_d(DD x, double d) {
#pragma clang fp contract(off) reassociate(off)
    const double q1 = x.hi / d;
    DD p = dd_two_prod(q1, d);
    DD r = dd_add(x, {-p.hi, -p.lo});
    const double q2 = r.hi / d;
    p = dd_two_prod(q2, d);
    r = dd_add(r, {-p.hi, -p.lo});
    const double q3 = r.hi / d;
    const DD q = dd_fast_two_sum(q1, q2);
    return dd_add(q, {q3, 0.0});
}

// 6 B, B the uniform cubic B-spline's power-basis matrix (bweights): row j the
// coefficients of t^j over the four nodes
TORJ_HD int cell_basis6(int j, int b) {
    //            b = 0   1   2  3
    // j = 0:         1   4   1  0
    // j = 1:        -3   0   3  0
    // j = 2:         3  -6   3  0
    // j = 3:        -1   3  -3  1
    const int M[16] = {1, 4, 1, 0, -3, 0, 3, 0, 3, -6, 3, 0, -1, 3, -3, 1};
    return M[j * 4 + b];
}

// One (cell, field) record of the power table: the 16 entries
//   A_ji = (sum_b sum_a M_jb M_ia c_ba) / 36 / hR^i / hZ^j,   M = 6 B,
// of the cell whose first node is c00 (row stride rs doubles between nodes in Z,
// ns doubles between nodes in R), out[j * 4 + i].  The integer products M_jb M_ia
// c_ba are exact double-doubles; the sum, the division by 36 and the i + j
// divisions by hR, hZ run in double-double (>= 100 bits), and each entry is
// rounded to double once, at the end: within 1 ulp of the exact value plus
// 2^-80 of the sum of the terms' magnitudes (tests/test_cell_table_dd.py holds
// that against exact rational arithmetic).
TORJ_HD void cell_record(const double *__restrict__ c00, size_t rs, size_t ns, double hR, double hZ,
                         double *__restrict__ out) {
#pragma clang fp contract(off) reassociate(off)
    double c[16];
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int a = 0; a < 4; a++) c[b * 4 + a] = c00[(size_t)b * rs + (size_t)a * ns];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            DD acc = {0.0, 0.0};
#pragma unroll
            for (int b = 0; b < 4; b++)
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    const int m = cell_basis6(j, b) * cell_basis6(i, a);
                    if (m != 0) acc = dd_add(acc, dd_two_prod((double)m, c[b * 4 + a]));
                }
            acc = dd_div_d(acc, 36.0);
            for (int k = 0; k < i; k++) acc = dd_div_d(acc, hR);
            for (int k = 0; k < j; k++) acc = dd_div_d(acc, hZ);
            out[j * 4 + i] = acc.hi;
        }
}

// d_cellp from d_coef: one thread per (cell, field), field fastest, so thread
// t's record starts at cellp + 16 t and a wave writes 8 KiB of consecutive
// memory, each thread its own 128-byte line in eight 16-byte stores.
// (TORJ_CELLTAB_NO_KERNEL: a host-only build of cell_record, which has no device
// code object for a kernel to live in)
#ifndef TORJ_CELLTAB_NO_KERNEL
__global__ __launch_bounds__(256) void k_cell_table(const double *__restrict__ coef, Grid g,
                                                    double *__restrict__ cellp) {
    const long n_cells = (long)(g.nR - 1) * (g.nZ - 1);
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_cells * kCellNS) return;
    const long cell = t / kCellNS;
    const int f = (int)(t - cell * kCellNS);
    const int iZ = (int)(cell / (g.nR - 1)), iR = (int)(cell - (long)iZ * (g.nR - 1));
    const size_t mR = (size_t)g.nR + 2;
    double rec[16];
    cell_record(coef + ((size_t)iZ * mR + (size_t)iR) * kNF + f, mR * kNF, kNF, g.hR, g.hZ, rec);
    Dbl2 *o = reinterpret_cast<Dbl2 *>(cellp + (size_t)t * 16);
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = Dbl2{rec[2 * k], rec[2 * k + 1]};
}
#endif
