// mtgp_variants.h -- run-time flags lifted to compile-time constants (no HIP: host C++17 only).
//
// Every evaluator kernel is a template over a few booleans (TRAJ, NOISE, JIT, ERK ...).  A launch
// picks the instantiation from run-time flags: the wrappers below call one generic functor with a
// std::bool_constant / std::integral_constant per flag, so a call site names each constant and no
// bare true / false sits in a template argument list:
//
//   mtgp::ctl_variant<Env::kMask>(traj, noise, jit, [&](auto T, auto N, auto J) {
//     hipLaunchKernelGGL((k_ctl_dopri5<Env, NA, T(), N(), J()>), grid, block, 0, s, A);
//   });
//
// The wrapper, not the call site, fixes which run-time flag lands in which position; only the
// variants a call can reach are instantiated (tests/test_variants_host.py: the truth tables).
#pragma once
#include <type_traits>
#include <utility>

namespace mtgp {

// f(std::bool_constant<flags>...), the constants in the order of the flags
template <class F>
constexpr decltype(auto) with_flags(F&& f) {
  return std::forward<F>(f)();
}
template <class F, class... Rest>
constexpr decltype(auto) with_flags(F&& f, bool flag, Rest... rest) {
  return flag ? with_flags([&](auto... c) -> decltype(auto) { return f(std::true_type{}, c...); }, rest...)
              : with_flags([&](auto... c) -> decltype(auto) { return f(std::false_type{}, c...); }, rest...);
}

// one flag (ERK, Dopri5): f(std::bool_constant<flag>)
template <class F>
constexpr decltype(auto) with_flag(bool flag, F&& f) {
  return with_flags(std::forward<F>(f), flag);
}

// f(TRAJ, rest...).  kTrajOnly (an environment with kMask: the trajectory variants are the only
// ones built): TRAJ is true, and nothing is called when `traj` is not set.
template <bool kTrajOnly, class F, class... Rest>
constexpr void traj_variant(F&& f, bool traj, Rest... rest) {
  if constexpr (kTrajOnly) {
    if (traj) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  } else {
    with_flags(std::forward<F>(f), traj, rest...);
  }
}

// the control kernels' <..., TRAJ, NOISE, JIT>: f(TRAJ, NOISE, JIT)
template <bool kTrajOnly, class F>
constexpr void ctl_variant(bool traj, bool noise, bool jit, F&& f) {
  traj_variant<kTrajOnly>(std::forward<F>(f), traj, noise, jit);
}

// the control kernels that have interpreter variants only, <..., TRAJ, NOISE, false>: f(TRAJ, NOISE)
template <bool kTrajOnly, class F>
constexpr void ctl_interp_variant(bool traj, bool noise, F&& f) {
  traj_variant<kTrajOnly>(std::forward<F>(f), traj, noise);
}

// the SR kernels' <..., TRAJ, JIT>: f(TRAJ, JIT)
template <class F>
constexpr decltype(auto) sr_variant(bool traj, bool jit, F&& f) {
  return with_flags(std::forward<F>(f), traj, jit);
}

// f(std::integral_constant<int, V>) for the V of Vs... that equals v; the last V when none does
// (a switch whose `default:` is its last case)
template <int V, int... Vs, class F>
constexpr decltype(auto) int_variant(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) {
    return std::forward<F>(f)(std::integral_constant<int, V>{});
  } else {
    return v == V ? f(std::integral_constant<int, V>{}) : int_variant<Vs...>(v, std::forward<F>(f));
  }
}

}  // namespace mtgp
