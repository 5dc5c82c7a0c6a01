// torj_traj.hip -- the split pipeline's trajectory kernel k_traj_cell in a
// translation unit of its own, compiled without machine-level loop-invariant
// code motion (csrc/Makefile TRAJ_FLAGS; the note in torj_k_traj.hpp): the
// trajectory kernels' header and the instances torj_hip.hip launches.
#include <hip/hip_runtime.h>

#include "torj_math.hpp"
#include "torj_fitdepo.hpp"

using namespace torj;

#include "torj_args.hpp"
#include "torj_k_traj.hpp"

template __global__ void k_traj_cell<kDepoSamples, true>(TraceArgs, SplitArgs);
template __global__ void k_traj_cell<kDepoSamples, false>(TraceArgs, SplitArgs);
template __global__ void k_traj_cell<kDepoBinned, true>(TraceArgs, SplitArgs);
template __global__ void k_traj_cell<kDepoBinned, false>(TraceArgs, SplitArgs);
template __global__ void k_traj_cell<kDepoNone, true>(TraceArgs, SplitArgs);
template __global__ void k_traj_cell<kDepoNone, false>(TraceArgs, SplitArgs);
