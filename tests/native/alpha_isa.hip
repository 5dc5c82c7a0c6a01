// k_alpha_pts<false> (the uncounted Albajar alpha kernel of the split pipeline)
// alone in a translation unit, behind the headers torj_hip.hip includes ahead
// of it and in its order, so that its assembly can be read without compiling
// the whole library: the kernel's code is the library's instruction for
// instruction (only the block labels' numbers differ).  Test harness only
// (tests/test_alpha_resources.py); compiled to assembly, never run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "torj_math.hpp"
#include "torj_entry.hpp"
#include "torj_fitdepo.hpp"
#include "torj_warm.hpp"

using namespace torj;

#include "torj_host_util.hpp"
#include "torj_args.hpp"
#include "torj_k_fused.hpp"
#include "torj_k_alpha.hpp"

template __global__ void k_alpha_pts<false>(TraceArgs, SplitArgs, int);
