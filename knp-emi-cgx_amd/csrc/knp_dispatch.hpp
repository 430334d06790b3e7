// Run-time values -> template arguments of a kernel launch, in one place (host code only; no HIP includes, so that the host
// compiler alone can test it: tools/dispatch_check.cpp).  A launcher writes its launch line once, in a generic lambda:
//   with_lanes<2, 64>(lanes, [&](auto L) { hipLaunchKernelGGL((k_spmv<L(), ...>), dim3(nblocks((int64_t)n_rows * L())), ...); });
// The ranges in use: <2, 64> generic CSR rows, <2, 32> node-blocked rows and compact level-0 legs, <4, 32> node-graph kernels,
// <2, 16> compact prolongator rows.
#pragma once
#include <type_traits>
#include <utility>

// `lanes` if it is a power of two in [LO, HI), else HI: zero, negative, odd and too-large counts run the widest instantiation
template <int LO, int HI>
constexpr int clamp_lanes(int lanes) {
    static_assert(LO > 0 && (LO & (LO - 1)) == 0 && (HI & (HI - 1)) == 0 && LO <= HI, "powers of two, LO <= HI");
    return lanes >= LO && lanes < HI && (lanes & (lanes - 1)) == 0 ? lanes : HI;
}
// f(std::integral_constant<int, L>{}) once, L = clamp_lanes<LO, HI>(lanes): only LO, 2 LO, ..., HI are instantiated
template <int LO, int HI, typename F>
inline void with_lanes(int lanes, F&& f) {
    if constexpr (LO >= HI) f(std::integral_constant<int, HI>{});
    else if (lanes == LO) f(std::integral_constant<int, LO>{});
    else with_lanes<2 * LO, HI>(lanes, std::forward<F>(f));
}
template <typename F>
inline void with_flag(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// the two-valued integers (unroll 1 / 2, basis vectors at once 3 / 8, dimension 2 / 3), smaller value first: A if `first`, else B
template <int A, int B, typename F>
inline void with_either(bool first, F&& f) {
    if (first) f(std::integral_constant<int, A>{});
    else f(std::integral_constant<int, B>{});
}
