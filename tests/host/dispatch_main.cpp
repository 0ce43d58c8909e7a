// The launchers' dispatch (pytemdiags_amd/csrc/dispatch.hpp) on its own: the header needs no HIP.  usage: dispatch_main
// For every list of values: each listed value reaches its own constant; values below, between and above the list reach
// the last entry; the callable runs exactly once and its return value comes back.  The strict pair dispatch calls
// nothing for a pair that is not listed, the dtype dispatch nothing for a dtype that is neither TEMX_F64 nor TEMX_F32.
// Prints "lists=<n> probes=<n> pairs=<n> dtypes=<n>"; a failed check prints the case and exits 1.
// tests/test_dispatch_host.py builds it with AddressSanitizer + UBSan.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "../../pytemdiags_amd/csrc/dispatch.hpp"

using namespace temx;

static int probes = 0;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAILED %s: ", #cond);                  \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      std::exit(1);                                       \
    }                                                     \
  } while (0)

template <int... V>
static void check_list(const char* name, IntList<V...> list) {
  const std::vector<int> listed{V...};
  std::vector<int> probe{INT_MIN, -1, 0, listed.front() - 1, listed.back() + 1, 1000, INT_MAX};
  for (size_t i = 0; i < listed.size(); ++i) {
    probe.push_back(listed[i]);
    if (i + 1 < listed.size() && listed[i] + 1 < listed[i + 1]) probe.push_back(listed[i] + 1);     // between two entries
  }
  for (int v : probe) {
    bool is_listed = false;
    for (int l : listed) is_listed = is_listed || l == v;
    const int want = is_listed ? v : listed.back();
    int calls = 0, got = 0;
    const int ret = dispatch(list, v, [&](auto c) {
      static_assert(std::is_same<decltype(c), Int<decltype(c)::value>>::value, "the callable gets an integral_constant");
      ++calls;
      got = decltype(c)::value;
      return 7000 + got;
    });
    CHECK(calls == 1 && got == want && ret == 7000 + want, "%s: value %d -> constant %d (want %d), %d calls, returned %d", name, v,
          got, want, calls, ret);
    ++probes;
  }
}

int main() {
  check_list("TB", TBValues{});
  check_list("TBS", TBSValues{});
  check_list("dpw", DpwValues{});
  check_list("bin J", BinJValues{});
  check_list("bin KP", BinKPValues{});
  check_list("slices", SliceValues{});
  // the fallbacks, spelled out
  const auto value_for = [](auto list, int v) { return dispatch(list, v, [](auto c) { return (int)decltype(c)::value; }); };
  CHECK(value_for(TBValues{}, 5) == 16 && value_for(TBSValues{}, 3) == 8 && value_for(DpwValues{}, 3) == 4 &&
        value_for(BinJValues{}, 9) == 12 && value_for(BinKPValues{}, 17) == 64 && value_for(SliceValues{}, 1) == 4, "fallbacks");

  int pairs = 0;
  const int want_pairs[3][2] = {{7, 13}, {4, 8}, {2, 4}};
  for (int a = -1; a <= 17; ++a)
    for (int b = -1; b <= 17; ++b) {
      bool is_listed = false;
      for (const auto& w : want_pairs) is_listed = is_listed || (w[0] == a && w[1] == b);
      int calls = 0, ga = 0, gb = 0, rc = -99;
      const bool hit = dispatch_strict(OsPairs{}, a, b, rc, [&](auto p) {
        ++calls;
        ga = decltype(p)::first;
        gb = decltype(p)::second;
        return 100 * ga + gb;
      });
      if (is_listed) CHECK(hit && calls == 1 && ga == a && gb == b && rc == 100 * a + b, "pair (%d, %d): %d calls, rc %d", a, b, calls, rc);
      else CHECK(!hit && calls == 0 && rc == -99, "pair (%d, %d) is not listed: %d calls, rc %d", a, b, calls, rc);
      ++pairs;
    }
  int rc0 = -99;
  CHECK(!dispatch_strict(OsPairs{}, 8, 16, rc0, [](auto) { return 1; }) && !dispatch_strict(OsPairs{}, 7, 8, rc0, [](auto) { return 1; }) &&
        rc0 == -99, "(8, 16) and (7, 8) call nothing");

  int dtypes = 0;
  for (int dtype : {INT_MIN, -1, (int)TEMX_F64, (int)TEMX_F32, 2, 3, INT_MAX}) {
    int calls = 0, size = 0, rc = -99;
    const bool hit = dispatch_dtype(dtype, rc, [&](auto t) {
      using T = typename decltype(t)::type;
      static_assert(std::is_same<T, double>::value || std::is_same<T, float>::value, "double or float");
      ++calls;
      size = (int)sizeof(T);
      return 40 + size;
    });
    if (dtype == TEMX_F64) CHECK(hit && calls == 1 && size == 8 && rc == 48, "TEMX_F64: %d calls, size %d, rc %d", calls, size, rc);
    else if (dtype == TEMX_F32) CHECK(hit && calls == 1 && size == 4 && rc == 44, "TEMX_F32: %d calls, size %d, rc %d", calls, size, rc);
    else CHECK(!hit && calls == 0 && rc == -99, "dtype %d: %d calls, rc %d", dtype, calls, rc);
    ++dtypes;
  }
  std::printf("lists=6 probes=%d pairs=%d dtypes=%d\n", probes, pairs, dtypes);
  return 0;
}
