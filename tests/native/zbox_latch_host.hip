// Host build of the block zero box (torj_math.hpp ZBox, zero_box_add,
// zero_box_flag, zero_box_kill) for the two facts the trajectory kernel's
// dead-box latch (torj_k_traj.hpp traj_run) rests on: the flag never comes back
// once it is false, and the latched bookkeeping writes the unlatched flags.
// Test harness only (tests/test_zbox_latch_host.py).
#include "torj_math.hpp"

#include <vector>

extern "C" {
int zl_gamma_lin() { return TORJ_NODE_GAMMA_LIN; }

// nb sequences of k points each (point p of sequence b at b * k + p), added in
// order: final[b] = the flag of the whole sequence, first_false[b] = the
// length of the shortest prefix (1 .. k) whose flag is false, 0 if none, and
// back[b] = the length of the first prefix whose flag is true after a shorter
// one's was false, 0 if none (the monotonicity's counterexample)
void zl_prefix(int nb, int k, const double *lnTe, const double *Y, const double *Npar, const double *N2,
               int *final_flag, int *first_false, int *back) {
    for (int b = 0; b < nb; b++) {
        torj::ZBox zb;
        int ff = 0, bk = 0;
        bool f = true;
        for (int p = 0; p < k; p++) {
            const size_t i = (size_t)b * k + p;
            torj::zero_box_add(zb, lnTe[i], Y[i], Npar[i], N2[i]);
            f = torj::zero_box_flag(zb);
            if (!f && !ff) ff = p + 1;
            if (f && ff && !bk) bk = p + 1;
        }
        final_flag[b] = f ? 1 : 0;
        first_false[b] = ff;
        back[b] = bk;
    }
}

// traj_run's bookkeeping over `wave` lanes at a time (lane l of wave w is
// sequence w * wave + l): every trip of the loop adds `stride` points (a step's
// stages) to the box of each lane still in the loop -- trip len[b] is lane b's
// last, and unless it is the block's last too the lane breaks out of it (a
// stop) after its points were added and before the vote -- while the wave's
// boxes are live; after the trips listed in
// cad (counted from 1) the wave looks at the flags of the lanes still in the
// loop and, if none is true, kills their boxes and stops adding.  flag[b] =
// zero_box_flag of lane b's box at the end, as traj_run writes it; latched[b] =
// the trip at which lane b's box was killed, 0 if never.
void zl_latched(int nb, int k, int stride, int wave, int ncad, const int *cad, const int *len,
                const double *lnTe, const double *Y, const double *Npar, const double *N2, int *flag,
                int *latched) {
    const int trips_max = k / stride;
    for (int w0 = 0; w0 < nb; w0 += wave) {
        const int nl = nb - w0 < wave ? nb - w0 : wave;
        std::vector<torj::ZBox> zb(nl);
        bool zon = true;
        for (int l = 0; l < nl; l++) latched[w0 + l] = 0;
        for (int t = 0; t < trips_max; t++) {
            bool any_in = false;
            for (int l = 0; l < nl; l++) {
                if (t >= len[w0 + l]) continue;  // this lane has left the loop
                any_in = true;
                if (!zon) continue;
                for (int s = 0; s < stride; s++) {
                    const size_t i = (size_t)(w0 + l) * k + (size_t)t * stride + s;
                    torj::zero_box_add(zb[l], lnTe[i], Y[i], Npar[i], N2[i]);
                }
            }
            if (!any_in) break;
            // the lanes that go on to the next trip vote (a lane whose last trip
            // this was has left the loop before the latch is reached)
            bool due = false;
            for (int c = 0; c < ncad; c++) due = due || cad[c] == t + 1;
            if (!zon || !due) continue;
            bool any = false, voters = false;
            for (int l = 0; l < nl; l++)
                if (t + 1 < len[w0 + l] || (t + 1 == len[w0 + l] && t + 1 == trips_max)) {
                    voters = true;
                    any = any || torj::zero_box_flag(zb[l]);
                }
            if (voters && !any) {
                for (int l = 0; l < nl; l++)
                    if (t + 1 < len[w0 + l] || (t + 1 == len[w0 + l] && t + 1 == trips_max)) {
                        torj::zero_box_kill(zb[l]);
                        latched[w0 + l] = t + 1;
                    }
                zon = false;
            }
        }
        for (int l = 0; l < nl; l++) flag[w0 + l] = torj::zero_box_flag(zb[l]) ? 1 : 0;
    }
}
}
