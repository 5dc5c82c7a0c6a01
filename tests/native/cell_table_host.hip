// Host build of torj_celltab.hpp's cell_record (the function k_cell_table runs per
// (cell, field) on the device) and of torj_math.hpp's cell_power_table, over a whole
// plasma's interleaved node coefficients, for tests/test_cell_table_dd.py and
// tests/test_gpu_plasma_update.py.  Compiled with --offload-host-only.
#include <hip/hip_runtime.h>

#include "torj_math.hpp"

using namespace torj;

#define TORJ_CELLTAB_NO_KERNEL 1
#include "torj_celltab.hpp"

extern "C" {

int ct_nf(void) { return kNF; }
int ct_rec(void) { return kCellRec; }

// coef: (nR + 2) x (nZ + 2) nodes, kNF doubles each -> out: (nR - 1) x (nZ - 1) x kCellRec,
// the loop k_cell_table's threads run
void ct_record_table(const double *coef, int nR, int nZ, double hR, double hZ, double *out) {
    const size_t mR = (size_t)nR + 2;
    for (int iZ = 0; iZ < nZ - 1; iZ++)
        for (int iR = 0; iR < nR - 1; iR++)
            for (int f = 0; f < kCellNS; f++)
                cell_record(coef + ((size_t)iZ * mR + (size_t)iR) * kNF + f, mR * kNF, kNF, hR, hZ,
                            out + (((size_t)iZ * (nR - 1) + iR) * kCellNS + f) * 16);
}

void ct_host_table(const double *coef, int nR, int nZ, double hR, double hZ, double *out) {
    cell_power_table(coef, nR, nZ, hR, hZ, out);
}

}  // extern "C"
