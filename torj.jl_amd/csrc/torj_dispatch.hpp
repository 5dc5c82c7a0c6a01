// torj_dispatch.hpp -- a launch's run-time (absorption, deposition mode,
// trajectory) as compile-time constants: the callee is a generic lambda that
// names its kernel instance from them, `if constexpr` where none may exist.
// (a slice of torj_hip.hip: included after `using namespace torj`)
#pragma once
#include <type_traits>

#include "torj_args.hpp"

template <int V>
using IntC = std::integral_constant<int, V>;

// f(IntC<absorption>): 0 cold, 1 Albajar, 2 / 3 the warm models
template <class F>
static void with_abs(int absorption, F f) {
    switch (absorption) {
    case 3: return f(IntC<3>{});
    case 2: return f(IntC<2>{});
    case 1: return f(IntC<1>{});
    default: return f(IntC<0>{});
    }
}

// f(IntC<DM>, std::bool_constant<tr>): the six (deposition mode, trajectory) pairs
template <class F>
static void with_depo_traj(int DM, bool tr, F f) {
    auto t = [&](auto D) { tr ? f(D, std::true_type{}) : f(D, std::false_type{}); };
    DM == kDepoBinned ? t(IntC<kDepoBinned>{}) : DM == kDepoSamples ? t(IntC<kDepoSamples>{}) : t(IntC<kDepoNone>{});
}

// f(IntC<absorption>, IntC<DM>, std::bool_constant<tr>)
template <class F>
static void with_abs_depo_traj(int absorption, int DM, bool tr, F f) {
    with_abs(absorption, [&](auto A) { with_depo_traj(DM, tr, [&](auto D, auto T) { f(A, D, T); }); });
}
