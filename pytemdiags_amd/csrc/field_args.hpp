// field_args.hpp -- host: the argument rules of the plan-free entry points (temxv_interp, temxl_to_engine,
// temxi_records_to_pressure, temxc_time_sum, temxn_time_sum_valid, temxg_time_sum_groups,
// temxw_time_sum_groups_valid), written once, and the level tables two of them share.  No HIP.
// A check returns a Refusal, which is true when the call is refused; the entry point hands its code and message to
// fail().  Every refusal here is TEMX_EINVAL.  tests/host/field_args_main.cpp runs this header under the sanitizers.
#ifndef TEMX_FIELD_ARGS_HPP
#define TEMX_FIELD_ARGS_HPP
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/temx_vert.h"

namespace temx {

struct Refusal {
  int code = TEMX_OK;
  char msg[200] = "";
  explicit operator bool() const { return code != TEMX_OK; }
};

__attribute__((format(printf, 1, 2))) inline Refusal refuse(const char* fmt, ...) {
  Refusal r{TEMX_EINVAL, ""};
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(r.msg, sizeof r.msg, fmt, ap);
  va_end(ap);
  return r;
}

// a | b: the first refusal of the two.  Both are evaluated, so chain only checks that read no memory (the scalar rules).
inline Refusal operator|(const Refusal& a, const Refusal& b) { return a ? a : b; }

inline Refusal check_nf(int nf, int nf_max) {
  return nf < 1 || nf > nf_max ? refuse("nf must lie in 1..%d, got %d", nf_max, nf) : Refusal{};
}
inline Refusal check_null(const void* p, const char* name) { return p ? Refusal{} : refuse("%s is null", name); }
inline Refusal check_dtype(int dtype, const char* name) {
  return dtype != TEMX_F64 && dtype != TEMX_F32 ? refuse("%s must be TEMX_F64 or TEMX_F32", name) : Refusal{};
}
inline Refusal check_flags(int flags, int known) {
  return flags & ~known ? refuse("flags has unknown bits (0x%x)", (unsigned)flags) : Refusal{};
}
inline Refusal check_method_edge(int method, int edge) {
  if (method != TEMXV_LOG && method != TEMXV_LINEAR) return refuse("method must be TEMXV_LOG or TEMXV_LINEAR");
  return edge != TEMXV_EDGE_NAN && edge != TEMXV_EDGE_HOLD ? refuse("edge must be TEMXV_EDGE_NAN or TEMXV_EDGE_HOLD") : Refusal{};
}

// nt_name: "nt" or "nt_src".  remap: a vertical remap, from nlev >= 2 levels to nplev.  Each size has a range, and
// ncol * levels * nt stays within 2^48, so that no byte count of a field comes near 2^64.
inline Refusal check_sizes(int64_t ncol, int nlev, int64_t nt, const char* nt_name, bool remap = false, int nplev = 1) {
  if (remap && (ncol < 1 || nt < 1 || nplev < 1 || nlev < 2)) return refuse("sizes must be positive (nlev at least 2)");
  if (ncol < 1) return refuse("ncol must be at least 1");
  if (nlev < 1) return refuse("nlev must be at least 1");
  if (nt < 1) return refuse("%s must be at least 1", nt_name);
  if (nlev > (1 << 20) || nplev > (1 << 20) || nt > (int64_t(1) << 31) || ncol > (int64_t(1) << 40))
    return refuse("sizes out of range (ncol, nlev%s or %s)", remap ? ", nplev" : "", nt_name);
  if ((double)ncol * (double)std::max(nlev, nplev) * (double)nt > 281474976710656.0)
    return refuse("sizes out of range (ncol * %s * %s above 2^48)", remap ? "levels" : "nlev", nt_name);
  return {};
}

// the window t0 .. t0 + ntb of a record of nt_src, which check_sizes has seen
inline Refusal check_window(int64_t nt_src, int64_t t0, int64_t ntb, bool remap = false) {
  if (ntb < 1) return remap ? refuse("sizes must be positive (nlev at least 2)") : refuse("ntb must be at least 1");
  if (t0 < 0) return refuse("t0 must not be negative");
  if (ntb > nt_src || t0 > nt_src - ntb)
    return refuse("t0 + ntb = %lld exceeds nt_src = %lld", (long long)((uint64_t)t0 + (uint64_t)ntb), (long long)nt_src);
  return {};
}

// the group arguments of temxg_time_sum_groups: ng groups, the block t0 .. t0 + nt (check_sizes has seen nt) of a record
// of nt_record times, one label per time of the record (-1: left out) and one weight, or weight null: all ones
inline Refusal check_groups(int ng, int ng_max, int64_t nt_record, int64_t t0, int64_t nt, const int32_t* label,
                            const double* weight) {
  if (ng < 1 || ng > ng_max) return refuse("ng must lie in 1..%d, got %d", ng_max, ng);
  if (!label) return refuse("label_host is null");
  if (t0 < 0) return refuse("t0 must not be negative");
  if (nt_record > INT32_MAX) return refuse("sizes out of range (nt_record above 2^31 - 1)");
  if (nt > nt_record || t0 > nt_record - nt)
    return refuse("t0 + nt = %lld exceeds nt_record = %lld", (long long)((uint64_t)t0 + (uint64_t)nt), (long long)nt_record);
  for (int64_t t = 0; t < nt_record; ++t)
    if (label[t] < -1 || label[t] >= ng)
      return refuse("label %lld is %d: labels lie in -1..%d", (long long)t, (int)label[t], ng - 1);
  for (int64_t t = 0; weight && t < nt_record; ++t)
    if (!std::isfinite(weight[t]) || weight[t] < 0.0)
      return refuse("weight %lld must be finite and not negative", (long long)t);
  return {};
}

// plev [nplev]; hyam, hybm [nlev] and p0, or hyam null: no hybrid coefficients (the pressure is a field)
inline Refusal check_levels(int nplev, const double* plev, int nlev, const double* hyam, const double* hybm, double p0) {
  if (hyam && !std::isfinite(p0)) return refuse("p0_hybrid is not finite");
  for (int j = 0; j < nplev; ++j)
    if (!(plev[j] > 0.0) || !std::isfinite(plev[j]) || (j && !(plev[j] > plev[j - 1])))
      return refuse("plev must be positive, finite and strictly ascending (entry %d)", j);
  for (int k = 0; hyam && k < nlev; ++k)
    if (!std::isfinite(hyam[k]) || !std::isfinite(hybm[k])) return refuse("hyam / hybm entry %d is not finite", k);
  return {};
}

inline size_t dtype_size(int dtype) { return dtype == TEMX_F64 ? 8 : 4; }

// do [a, a + na) and [b, b + nb) share a byte?  na, nb > 0.  Nothing is added to an address, so nothing wraps: an extent
// that would end beyond the top of the address space counts as reaching it.  Touching extents do not overlap.
inline bool extents_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y ? y - x < na : x - y < nb;
}

// nf inputs of src_elems elements, input f of src_dtype[f]; nf outputs ("dst" or "acc") of out_elems elements of out_dtype;
// one more input (ps) of extra_elems elements of extra_dtype, or null: none
struct FieldSet {
  int nf;
  const void* const* src; const int* src_dtype; size_t src_elems;
  void* const* out; const char* out_name; int out_dtype; size_t out_elems;
  const void* extra; const char* extra_name; int extra_dtype; size_t extra_elems;
};

// per field: dtype, no narrowing, null, alignment; then every output against the extra input, every input, every earlier output
inline Refusal check_fields(const FieldSet& a) {
  const size_t out_bytes = a.out_elems * dtype_size(a.out_dtype);
  if (a.extra && (uintptr_t)a.extra % dtype_size(a.extra_dtype)) return refuse("%s is not aligned to its element size", a.extra_name);
  for (int f = 0; f < a.nf; ++f) {
    if (a.src_dtype[f] != TEMX_F64 && a.src_dtype[f] != TEMX_F32) return refuse("src_dtype %d must be TEMX_F64 or TEMX_F32", f);
    if (a.src_dtype[f] == TEMX_F64 && a.out_dtype == TEMX_F32)
      return refuse("src_dtype %d is TEMX_F64 but %s_dtype is TEMX_F32: this call does not narrow", f, a.out_name);
    if (!a.src[f]) return refuse("src %d is null", f);
    if (!a.out[f]) return refuse("%s %d is null", a.out_name, f);
    if ((uintptr_t)a.src[f] % dtype_size(a.src_dtype[f])) return refuse("src %d is not aligned to its element size", f);
    if ((uintptr_t)a.out[f] % dtype_size(a.out_dtype)) return refuse("%s %d is not aligned to its element size", a.out_name, f);
  }
  for (int f = 0; f < a.nf; ++f) {
    if (a.extra && extents_overlap(a.out[f], out_bytes, a.extra, a.extra_elems * dtype_size(a.extra_dtype)))
      return refuse("%s %d overlaps %s", a.out_name, f, a.extra_name);
    for (int g = 0; g < a.nf; ++g) {
      if (extents_overlap(a.out[f], out_bytes, a.src[g], a.src_elems * dtype_size(a.src_dtype[g])))
        return refuse("%s %d overlaps src %d", a.out_name, f, g);
      if (g < f && extents_overlap(a.out[f], out_bytes, a.out[g], out_bytes))
        return refuse("%s %d overlaps %s %d", a.out_name, f, a.out_name, g);
    }
  }
  return {};
}

// temxn_time_sum_valid: nf inputs of one dtype, nf fp64 accumulators and ncnt fp64 counts (nf, or 1 under a common mask),
// outputs of out_elems elements each.  The accumulators go by check_fields; a count obeys the rules of an accumulator
// and overlaps no accumulator either.
inline Refusal check_sum_valid(int nf, const void* const* src, int dtype, size_t src_elems, double* const* acc,
                               double* const* cnt, int ncnt, size_t out_elems) {
  int dts[16];
  for (int f = 0; f < nf && f < 16; ++f) dts[f] = dtype;
  if (Refusal r = check_fields({nf, src, dts, src_elems, (void* const*)acc, "acc", TEMX_F64, out_elems})) return r;
  const size_t out_bytes = out_elems * sizeof(double);
  for (int f = 0; f < ncnt; ++f) {
    if (!cnt[f]) return refuse("cnt %d is null", f);
    if ((uintptr_t)cnt[f] % sizeof(double)) return refuse("cnt %d is not aligned to its element size", f);
  }
  for (int f = 0; f < ncnt; ++f)
    for (int g = 0; g < nf; ++g) {
      if (extents_overlap(cnt[f], out_bytes, src[g], src_elems * dtype_size(dtype))) return refuse("cnt %d overlaps src %d", f, g);
      if (extents_overlap(cnt[f], out_bytes, acc[g], out_bytes)) return refuse("cnt %d overlaps acc %d", f, g);
      if (g < f && extents_overlap(cnt[f], out_bytes, cnt[g], out_bytes)) return refuse("cnt %d overlaps cnt %d", f, g);
    }
  return {};
}

// temxw_time_sum_groups_valid: as check_sum_valid, with two further sets of nextra fp64 outputs (nf, or 1 under a common
// mask), the weight sums and the counts.  Each obeys the rules of an accumulator and overlaps no source and no other output.
// (tests/host/mgclim_shapes_main.cpp runs this check under the sanitizers.)
inline Refusal check_sum_groups_valid(int nf, const void* const* src, int dtype, size_t src_elems, double* const* acc,
                                      double* const* wsum, double* const* cnt, int nextra, size_t out_elems) {
  if (Refusal r = check_sum_valid(nf, src, dtype, src_elems, acc, cnt, nextra, out_elems)) return r;
  const size_t out_bytes = out_elems * sizeof(double);
  for (int f = 0; f < nextra; ++f) {
    if (!wsum[f]) return refuse("wsum %d is null", f);
    if ((uintptr_t)wsum[f] % sizeof(double)) return refuse("wsum %d is not aligned to its element size", f);
  }
  for (int f = 0; f < nextra; ++f) {
    for (int g = 0; g < nf; ++g) {
      if (extents_overlap(wsum[f], out_bytes, src[g], src_elems * dtype_size(dtype))) return refuse("wsum %d overlaps src %d", f, g);
      if (extents_overlap(wsum[f], out_bytes, acc[g], out_bytes)) return refuse("wsum %d overlaps acc %d", f, g);
    }
    for (int g = 0; g < nextra; ++g) {
      if (extents_overlap(wsum[f], out_bytes, cnt[g], out_bytes)) return refuse("wsum %d overlaps cnt %d", f, g);
      if (g < f && extents_overlap(wsum[f], out_bytes, wsum[g], out_bytes)) return refuse("wsum %d overlaps wsum %d", f, g);
    }
  }
  return {};
}

inline unsigned f32_mask(int nf, const int* src_dtype) {   // bit f: input f is fp32
  unsigned m = 0;
  for (int f = 0; f < nf; ++f) m |= (src_dtype[f] == TEMX_F32 ? 1u : 0u) << f;
  return m;
}

// the level tables of a remap as they are uploaded: [hyam | hybm] (unless hyam is null) | plev | ln plev or plev | method.
// temxv_interp and temxi_records_to_pressure go through one cache with it (vert_tables): equal levels, equal vector.
inline std::vector<double> vert_table_host(int nlev, const double* hyam, const double* hybm, int nplev, const double* plev,
                                           int method) {
  std::vector<double> host;
  host.reserve((hyam ? 2 * (size_t)nlev : 0) + 2 * (size_t)nplev + 1);
  if (hyam) {
    host.insert(host.end(), hyam, hyam + nlev);
    host.insert(host.end(), hybm, hybm + nlev);
  }
  host.insert(host.end(), plev, plev + nplev);
  for (int j = 0; j < nplev; ++j) host.push_back(method == TEMXV_LOG ? std::log(plev[j]) : plev[j]);
  host.push_back((double)method);
  return host;
}

}  // namespace temx

#endif
