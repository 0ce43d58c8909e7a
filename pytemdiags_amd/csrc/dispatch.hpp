// dispatch.hpp -- host: how a launcher turns a runtime value into a template argument, written once.  No HIP.
// Every list of values the kernels are instantiated for stands here; dispatch() hands the callable a
// std::integral_constant for the entry that matches, and the LAST entry for every other value (the plan builder only
// produces listed values; the last entry is the widest instantiation).  The callable runs exactly once and its int
// comes back.  tests/host/dispatch_main.cpp runs this header under the sanitizers.
#ifndef TEMX_DISPATCH_HPP
#define TEMX_DISPATCH_HPP
#include <type_traits>

#include "../../include/temx.h"

namespace temx {

template <int V> using Int = std::integral_constant<int, V>;
template <int... V> struct IntList {};
template <int A, int B> struct IntPair { static constexpr int first = A, second = B; };
template <typename... P> struct PairList {};
template <typename T> struct TypeTag { using type = T; };

using TBValues = IntList<4, 8, 13, 16>;          // 4x4 blocks of harmonics per group, generic sweeps (K <= 64)
using TBSValues = IntList<2, 4, 7, 8>;           // blocks per parity, class and pair sweeps
using DpwValues = IntList<1, 2, 4>;              // d-tiles per workgroup
using BinJValues = IntList<8, 10, 12>;           // Chebyshev terms per latitude bin
using BinKPValues = IntList<16, 32, 48, 64>;     // K rounded up to a multiple of 16, binned form
using SliceValues = IntList<2, 3, 4>;            // slices of 64 harmonics, large-L class path
using GclimBoundValues = IntList<1, 4, 64>;      // groups present in a block, grouped time sum on long rows (64: any)
using OsPairs = PairList<IntPair<7, 13>, IntPair<4, 8>, IntPair<2, 4>>;   // single sweep: (TBS, TBX)

template <int V0, int... Vs, typename F>
int dispatch(IntList<V0, Vs...>, int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) return f(Int<V0>{});
  else return v == V0 ? f(Int<V0>{}) : dispatch(IntList<Vs...>{}, v, f);
}

// strict: a pair that is not listed calls nothing and returns false; otherwise rc = f(the pair)
template <typename F>
bool dispatch_strict(PairList<>, int, int, int&, F&&) { return false; }
template <typename P0, typename... Ps, typename F>
bool dispatch_strict(PairList<P0, Ps...>, int a, int b, int& rc, F&& f) {
  if (a != P0::first || b != P0::second) return dispatch_strict(PairList<Ps...>{}, a, b, rc, f);
  rc = f(P0{});
  return true;
}

// rc = f(TypeTag<double or float>); false, and no call, for any other dtype
template <typename F>
bool dispatch_dtype(int dtype, int& rc, F&& f) {
  if (dtype == TEMX_F64) rc = f(TypeTag<double>{});
  else if (dtype == TEMX_F32) rc = f(TypeTag<float>{});
  else return false;
  return true;
}

}  // namespace temx
#endif
