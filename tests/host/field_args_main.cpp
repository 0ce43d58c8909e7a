// The argument rules of the plan-free entry points (pytemdiags_amd/csrc/field_args.hpp) on their own: the header needs
// no HIP.  usage: field_args_main
// (a) the aliasing check of check_fields: for nf = 1..8, both element sizes, every pair of extents the check compares
//     (an output and the extra input, an output and an input, an output and an earlier output), and once no pair at all; a
//     pair is placed nine ways (disjoint, touching, overlapping by one element, nested, on either side) at the bottom, in
//     the middle and at the very top of the address space, every other extent well apart; the answer and its text must be
//     those of an interval test in 128-bit arithmetic that walks the pairs in the documented order.
// (b) vert_table_host: [hyam | hybm | plev | ln plev or plev | method] for nlev = 2, 3, 72, nplev = 1, 2, 30 and both
//     methods, and the same without hyam and hybm.  temxv_interp in hybrid mode and temxi_records_to_pressure both call
//     it with these arguments, so equal levels give them equal vectors.
// (c) the scalar rules at the ends of their argument ranges, for UBSan.
// (d) check_fields on two fields of mixed element sizes (an fp32 and an fp64 source, fp64 or fp32 outputs, an fp32 extra
//     input): the per-field dtype, narrowing, null and alignment rules, and extents sized by each array's own dtype.
// Prints "alias_cases=<n> refused=<n> table_cases=<n> mixed_cases=<n>"; a failed check prints the case and exits 1.
// tests/test_field_args_host.py builds it with AddressSanitizer + UBSan.
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../pytemdiags_amd/csrc/field_args.hpp"

typedef unsigned __int128 u128;

static const size_t SRC_ELEMS = 12, OUT_ELEMS = 5, EXTRA_ELEMS = 7;

static bool overlap128(uintptr_t a, size_t na, uintptr_t b, size_t nb) {
  return (u128)a < (u128)b + nb && (u128)b < (u128)a + na;
}

// what check_fields must say about aligned, non-null extents: "" or the first overlapping pair in its order
static std::string expected(int nf, const std::vector<uintptr_t>& src, const std::vector<uintptr_t>& out, uintptr_t extra,
                            size_t esz) {
  char buf[64];
  for (int f = 0; f < nf; ++f) {
    if (overlap128(out[f], OUT_ELEMS * esz, extra, EXTRA_ELEMS * esz)) {
      std::snprintf(buf, sizeof buf, "dst %d overlaps ps", f);
      return buf;
    }
    for (int g = 0; g < nf; ++g) {
      if (overlap128(out[f], OUT_ELEMS * esz, src[g], SRC_ELEMS * esz)) {
        std::snprintf(buf, sizeof buf, "dst %d overlaps src %d", f, g);
        return buf;
      }
      if (g < f && overlap128(out[f], OUT_ELEMS * esz, out[g], OUT_ELEMS * esz)) {
        std::snprintf(buf, sizeof buf, "dst %d overlaps dst %d", f, g);
        return buf;
      }
    }
  }
  return "";
}

int main() {
  long long alias_cases = 0, refused = 0, table_cases = 0;
  for (int nf = 1; nf <= 8; ++nf)
    for (size_t esz : {(size_t)8, (size_t)4}) {
      const int dtype = esz == 8 ? TEMX_F64 : TEMX_F32;
      const std::vector<int> sdt((size_t)nf, dtype);
      // the pairs: kind 0 none, 1 out f / extra, 2 out f / src g, 3 out f / out g (g < f)
      struct Pair { int kind, f, g; };
      std::vector<Pair> pairs{{0, 0, 0}};
      for (int f = 0; f < nf; ++f) {
        pairs.push_back({1, f, 0});
        for (int g = 0; g < nf; ++g) pairs.push_back({2, f, g});
        for (int g = 0; g < f; ++g) pairs.push_back({3, f, g});
      }
      for (const Pair& pr : pairs) {
        const size_t nb = OUT_ELEMS * esz;                                      // the output that is moved
        const size_t na = (pr.kind == 1 ? EXTRA_ELEMS : pr.kind == 2 ? SRC_ELEMS : OUT_ELEMS) * esz;   // what it is moved against
        // offset of the output from the other extent, in bytes
        const long long offs[9] = {-(long long)nb - 3 * (long long)esz, -(long long)nb, -(long long)nb + (long long)esz,
                                   -(long long)esz, 0, (long long)esz, (long long)na - (long long)esz, (long long)na,
                                   (long long)na + 3 * (long long)esz};
        for (int base = 0; base < (pr.kind ? 3 : 1); ++base)
          for (long long off : offs) {
            if (!pr.kind && off != offs[0]) break;      // nothing is moved: once
            // every extent apart, 4096 bytes from the next, in the middle of the address space
            std::vector<uintptr_t> src((size_t)nf), out((size_t)nf);
            for (int f = 0; f < nf; ++f) {
              src[(size_t)f] = ((uintptr_t)1 << 40) + (uintptr_t)f * 4096;
              out[(size_t)f] = ((uintptr_t)1 << 41) + (uintptr_t)f * 4096;
            }
            uintptr_t extra = (uintptr_t)1 << 42;
            if (pr.kind) {
              // the lower of the two extents starts at 8 (base 0), or the higher one ends at 2^64 (base 2)
              const long long hi = std::max((long long)na, off + (long long)nb);      // the end of the higher one, from a
              const uintptr_t a = base == 0 ? (uintptr_t)(8 + (off < 0 ? -off : 0)) : base == 1 ? (uintptr_t)1 << 50
                                                                                                : (uintptr_t)0 - (uintptr_t)hi;
              const uintptr_t b = a + (uintptr_t)off;                                  // in range by construction
              out[(size_t)pr.f] = b;
              if (pr.kind == 1) extra = a;
              else if (pr.kind == 2) src[(size_t)pr.g] = a;
              else out[(size_t)pr.g] = a;
            }
            const temx::FieldSet fs{nf, (const void* const*)src.data(), sdt.data(), SRC_ELEMS, (void* const*)out.data(), "dst",
                                    dtype, OUT_ELEMS, (const void*)extra, "ps", dtype, EXTRA_ELEMS};
            const temx::Refusal r = temx::check_fields(fs);
            const std::string want = expected(nf, src, out, extra, esz);
            ++alias_cases;
            refused += r ? 1 : 0;
            if (want != r.msg || (r.code != (want.empty() ? TEMX_OK : TEMX_EINVAL))) {
              std::printf("FAILED alias nf=%d esz=%zu kind=%d f=%d g=%d base=%d off=%lld: got \"%s\" want \"%s\"\n", nf, esz,
                          pr.kind, pr.f, pr.g, base, off, r.msg, want.c_str());
              return 1;
            }
          }
      }
    }

  for (int nlev : {2, 3, 72})
    for (int nplev : {1, 2, 30})
      for (int method : {(int)TEMXV_LOG, (int)TEMXV_LINEAR}) {
        std::vector<double> hyam((size_t)nlev), hybm((size_t)nlev), plev((size_t)nplev);
        for (int k = 0; k < nlev; ++k) hyam[(size_t)k] = 0.001 * (k + 1), hybm[(size_t)k] = 0.5 + 0.002 * k;
        for (int j = 0; j < nplev; ++j) plev[(size_t)j] = 100.0 * (j + 1) * (j + 1);
        std::vector<double> want(hyam);
        want.insert(want.end(), hybm.begin(), hybm.end());
        want.insert(want.end(), plev.begin(), plev.end());
        for (double p : plev) want.push_back(method == TEMXV_LOG ? std::log(p) : p);
        want.push_back((double)method);
        const std::vector<double> hybrid = temx::vert_table_host(nlev, hyam.data(), hybm.data(), nplev, plev.data(), method);
        const std::vector<double> field = temx::vert_table_host(nlev, nullptr, nullptr, nplev, plev.data(), method);
        ++table_cases;
        if (hybrid.size() != 2 * (size_t)nlev + 2 * (size_t)nplev + 1 || field.size() != 2 * (size_t)nplev + 1 ||
            std::memcmp(hybrid.data(), want.data(), want.size() * sizeof(double)) ||
            std::memcmp(field.data(), want.data() + 2 * nlev, field.size() * sizeof(double)) ||
            temx::check_levels(nplev, plev.data(), nlev, hyam.data(), hybm.data(), 1e5)) {
          std::printf("FAILED tables nlev=%d nplev=%d method=%d\n", nlev, nplev, method);
          return 1;
        }
      }

  // the scalar rules at the ends of their ranges: nothing here may overflow
  const int64_t big = INT64_MAX, small = INT64_MIN;
  const bool ends = temx::check_window(5, big, 2) && temx::check_window(5, 1, big) && temx::check_window(small, 0, 1) &&
                    temx::check_window(big, big, big) && !temx::check_window(big, 0, big) && temx::check_window(5, small, 1) &&
                    temx::check_sizes(big, INT_MAX, big, "nt") && temx::check_sizes(small, INT_MIN, small, "nt", true, INT_MIN) &&
                    temx::check_sizes(1, 1, 1, "nt", true, 1) && !temx::check_sizes((int64_t)1 << 40, 1 << 8, 1, "nt") &&
                    temx::check_sizes(((int64_t)1 << 40), 1 << 8, 2, "nt") && temx::check_flags(INT_MIN, 1) &&
                    temx::check_nf(INT_MIN, 8) && temx::check_dtype(INT_MAX, "dtype") && temx::check_method_edge(0, INT_MIN) &&
                    (temx::check_nf(0, 8) | temx::check_dtype(7, "dtype")).msg[0] == 'n' &&
                    (temx::check_nf(1, 8) | temx::check_dtype(7, "dtype")).msg[0] == 'd' &&
                    temx::f32_mask(3, std::vector<int>{TEMX_F32, TEMX_F64, TEMX_F32}.data()) == 5u;
  if (!ends) {
    std::printf("FAILED scalar rules\n");
    return 1;
  }
  // two fields of mixed element sizes: src 0 fp32 (48 bytes), src 1 fp64 (96 bytes), outputs of 5 elements, extra fp32 (28 bytes)
  const uintptr_t S0 = 1 << 20, S1 = 2 << 20, O0 = 3 << 20, O1 = 4 << 20, X = 5 << 20;
  const int F64 = TEMX_F64, F32 = TEMX_F32;
  struct Mixed { uintptr_t src[2]; int sdt[2]; uintptr_t out[2]; int odt; uintptr_t extra; const char* want; };
  const Mixed mixed[] = {
      {{S0, S1}, {F32, F64}, {O0, O1}, F64, X, ""},
      {{S0, S1}, {F32, F32}, {O0, O1}, F32, X, ""},
      {{S0, S1}, {F32, 7}, {O0, O1}, F64, X, "src_dtype 1 must be TEMX_F64 or TEMX_F32"},
      {{S0, S1}, {-1, F64}, {O0, O1}, F64, X, "src_dtype 0 must be TEMX_F64 or TEMX_F32"},
      {{S0, S1}, {F32, F64}, {O0, O1}, F32, X, "src_dtype 1 is TEMX_F64 but dst_dtype is TEMX_F32: this call does not narrow"},
      {{S0, 0}, {F32, F64}, {O0, O1}, F64, X, "src 1 is null"},
      {{S0, S1}, {F32, F64}, {0, O1}, F64, X, "dst 0 is null"},
      {{S0 + 4, S1}, {F32, F64}, {O0, O1}, F64, X, ""},
      {{S0 + 2, S1}, {F32, F64}, {O0, O1}, F64, X, "src 0 is not aligned to its element size"},
      {{S0, S1 + 4}, {F32, F64}, {O0, O1}, F64, X, "src 1 is not aligned to its element size"},
      {{S0, S1}, {F32, F64}, {O0, O1 + 4}, F64, X, "dst 1 is not aligned to its element size"},
      {{S0, S1}, {F32, F32}, {O0, O1 + 4}, F32, X, ""},
      {{S0, S1}, {F32, F64}, {O0, O1}, F64, X + 4, ""},
      {{S0, S1}, {F32, F64}, {O0, O1}, F64, X + 2, "ps is not aligned to its element size"},
      {{S0, S1}, {F32, F64}, {S0 + 48, O1}, F64, X, ""},                          // behind the 48 bytes of the fp32 source
      {{S0, S1}, {F32, F64}, {S0 + 40, O1}, F64, X, "dst 0 overlaps src 0"},
      {{S0, S1}, {F32, F64}, {O0, S1 + 96}, F64, X, ""},                          // behind the 96 bytes of the fp64 source
      {{S0, S1}, {F32, F64}, {O0, S1 + 88}, F64, X, "dst 1 overlaps src 1"},
      {{S0, S1}, {F32, F64}, {X + 32, O1}, F64, X, ""},                           // behind the 28 bytes of the extra input
      {{S0, S1}, {F32, F64}, {X + 24, O1}, F64, X, "dst 0 overlaps ps"},
      {{S0, S1}, {F32, F32}, {O0, O0 + 20}, F32, X, ""},                          // fp32 outputs are 20 bytes
      {{S0, S1}, {F32, F32}, {O0, O0 + 16}, F32, X, "dst 1 overlaps dst 0"},
      {{S0, S1}, {F32, F64}, {O0, O0 + 32}, F64, X, "dst 1 overlaps dst 0"},      // fp64 outputs are 40
  };
  long long mixed_cases = 0;
  for (const Mixed& m : mixed) {
    const void* src[2] = {(const void*)m.src[0], (const void*)m.src[1]};
    void* out[2] = {(void*)m.out[0], (void*)m.out[1]};
    const temx::Refusal r = temx::check_fields({2, src, m.sdt, SRC_ELEMS, out, "dst", m.odt, OUT_ELEMS, (const void*)m.extra,
                                                "ps", F32, EXTRA_ELEMS});
    ++mixed_cases;
    if (std::strcmp(r.msg, m.want) || (r.code != (*m.want ? TEMX_EINVAL : TEMX_OK))) {
      std::printf("FAILED mixed case %lld: got \"%s\" want \"%s\"\n", mixed_cases - 1, r.msg, m.want);
      return 1;
    }
  }
  std::printf("alias_cases=%lld refused=%lld table_cases=%lld mixed_cases=%lld\n", alias_cases, refused, table_cases, mixed_cases);
  return 0;
}
