// gclim_tables.hpp -- host: the tables and launch shapes of the grouped time sum (kernels_gclim.hpp,
// include/temx_gclim.h).  Pure functions of the labels, the weights and sizes; no HIP.
//
// The record's table (GclimRecord) is built once per (labels, weights, ng) and uploaded once: the times of the record
// sorted by (group, time) with their weights, so that the times of a group inside any window [t0, t0 + nt) are one
// contiguous range of the sorted list, plus the raw labels and weights for the long-row kernel.  Left-out times (label
// -1) are in no group's range.  A call adds the small per-window part (GclimWindow), which travels in the kernel
// arguments: the groups present in the window and the range of each in the sorted list.
//
// Launch shapes are those of the plain time sum (clim_shapes.hpp: staged rows up to clim_switch_nt, a wave per row
// beyond), so they depend on (nt, element size) only; the long-row kernel has a register form for a few groups present
// and an LDS form for more (gclim_bound), which picks the kernel and no bit of the result.
#ifndef TEMX_GCLIM_TABLES_HPP
#define TEMX_GCLIM_TABLES_HPP
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "clim_shapes.hpp"

namespace temx {

constexpr int GCLIM_NFMAX = CLIM_NFMAX;
constexpr int GCLIM_NGMAX = 64;

// the record's table: the content key (what the caller gave) and the device image
struct GclimRecord {
  int ng = 0;
  int64_t nt_record = 0;
  std::vector<unsigned char> key;   // ng | nt_record | labels | has-weights | weights: equal records, equal keys
  std::vector<int32_t> start;       // [ng + 1]: group g owns sorted[start[g] .. start[g + 1])
  std::vector<int32_t> sorted;      // the labelled times by (group, time)
  // device image, in this order (the doubles first: every part keeps its alignment)
  //   w  [nt_record] doubles   the weights by time
  //   sw [nt_record] doubles   the weights in sorted order (entries beyond the labelled times are 0)
  //   lab[nt_record] int32     the labels by time
  //   st [nt_record] int32     the sorted times (entries beyond the labelled times are 0)
  std::vector<unsigned char> image;
  size_t off_w() const { return 0; }
  size_t off_sw() const { return (size_t)nt_record * 8; }
  size_t off_lab() const { return (size_t)nt_record * 16; }
  size_t off_st() const { return (size_t)nt_record * 20; }
};

inline std::vector<unsigned char> gclim_key(int ng, int64_t nt_record, const int32_t* label, const double* weight_or_null) {
  const size_t n = (size_t)nt_record;
  std::vector<unsigned char> k(16 + n * 4 + 8 + (weight_or_null ? n * 8 : 0));
  const int64_t head[2] = {ng, nt_record};
  std::memcpy(k.data(), head, 16);
  if (n) std::memcpy(k.data() + 16, label, n * 4);
  const int64_t has = weight_or_null ? 1 : 0;
  std::memcpy(k.data() + 16 + n * 4, &has, 8);
  if (weight_or_null && n) std::memcpy(k.data() + 24 + n * 4, weight_or_null, n * 8);
  return k;
}

// labels in -1 .. ng-1 (check_groups of field_args.hpp has seen them)
inline GclimRecord gclim_record(int ng, int64_t nt_record, const int32_t* label, const double* weight_or_null) {
  GclimRecord r;
  r.ng = ng;
  r.nt_record = nt_record;
  r.key = gclim_key(ng, nt_record, label, weight_or_null);
  const size_t n = (size_t)nt_record;
  r.start.assign((size_t)ng + 1, 0);
  for (size_t t = 0; t < n; ++t)
    if (label[t] >= 0) ++r.start[(size_t)label[t] + 1];
  for (int g = 0; g < ng; ++g) r.start[(size_t)g + 1] += r.start[(size_t)g];
  r.sorted.assign((size_t)r.start[(size_t)ng], 0);
  std::vector<int32_t> fill(r.start.begin(), r.start.end() - 1);
  for (size_t t = 0; t < n; ++t)       // (a counting sort: times stay ascending inside a group)
    if (label[t] >= 0) r.sorted[(size_t)fill[(size_t)label[t]]++] = (int32_t)t;
  std::vector<double> w(n, 1.0), sw(n, 0.0);
  if (weight_or_null) std::copy(weight_or_null, weight_or_null + n, w.begin());
  for (size_t j = 0; j < r.sorted.size(); ++j) sw[j] = w[(size_t)r.sorted[j]];
  std::vector<int32_t> st(n, 0);
  std::copy(r.sorted.begin(), r.sorted.end(), st.begin());
  r.image.assign(n * 24, 0);
  if (n) {
    std::memcpy(r.image.data() + r.off_w(), w.data(), n * 8);
    std::memcpy(r.image.data() + r.off_sw(), sw.data(), n * 8);
    std::memcpy(r.image.data() + r.off_lab(), label, n * 4);
    std::memcpy(r.image.data() + r.off_st(), st.data(), n * 4);
  }
  return r;
}

// the per-window part, small enough for the kernel arguments
struct GclimWindow {
  int np;                          // groups present in the window
  int ng;
  unsigned long long mask;         // bit g: group g is present
  int pg[GCLIM_NGMAX];             // the present groups, ascending; -2 beyond np (matches no label)
  int lo[GCLIM_NGMAX];             // present group q owns sorted[lo[q] .. hi[q]) inside the window, times ascending
  int hi[GCLIM_NGMAX];
};

inline GclimWindow gclim_window(const GclimRecord& r, int64_t t0, int64_t nt) {
  GclimWindow w{};
  w.ng = r.ng;
  for (int q = 0; q < GCLIM_NGMAX; ++q) w.pg[q] = -2;
  for (int g = 0; g < r.ng; ++g) {
    const int32_t* b = r.sorted.data() + r.start[(size_t)g];
    const int32_t* e = r.sorted.data() + r.start[(size_t)g + 1];
    const int32_t* lo = std::lower_bound(b, e, (int32_t)t0);
    const int32_t* hi = std::lower_bound(lo, e, (int32_t)(t0 + nt));   // t0 + nt <= nt_record <= 2^31 - 1
    if (hi > lo) {
      w.pg[w.np] = g;
      w.lo[w.np] = (int)(lo - r.sorted.data());
      w.hi[w.np] = (int)(hi - r.sorted.data());
      w.mask |= 1ull << g;
      ++w.np;
    }
  }
  return w;
}

// long rows: the register form of the kernel is instantiated for at most 1 and at most 4 groups present; with more, the
// accumulators live in LDS (GCLIM_NGMAX stands for "any number")
inline int gclim_bound(int np) { return np <= 1 ? 1 : np <= 4 ? 4 : GCLIM_NGMAX; }

constexpr int GCLIM_LONG_LDS_BYTES = 48 * 1024;   // LDS form of the long rows: the images of a workgroup's waves
// rows (waves) per workgroup of the LDS form: an image is ng * 64 doubles
inline int gclim_lds_rows(int ng) {
  const int fit = GCLIM_LONG_LDS_BYTES / (ng * 64 * 8);
  return fit < 1 ? 1 : fit < CLIM_LONG_ROWS ? fit : CLIM_LONG_ROWS;
}

// the launch of one dtype's fields: the cut of the rows into staged and long is that of the plain time sum, a function
// of (nt, element size); the groups present pick the form of the long-row kernel, and ng its rows per workgroup
struct GclimShape {
  ClimShape rows;
  int bound;         // long rows: gclim_bound(np); staged: 0
  int rpw;           // rows per workgroup (rows.rpb, or gclim_lds_rows(ng) in the LDS form of the long rows)
  int64_t nblk;      // workgroups of one field
  size_t lds_bytes;  // staged: bytes of the LDS image (<= CLIM_LDS_BYTES); LDS form: rpw images (<= GCLIM_LONG_LDS_BYTES)
};

inline GclimShape gclim_shape(int64_t rows, int64_t nt, size_t esz, int np, int ng) {
  GclimShape s{};
  s.rows = clim_shape(rows, nt, esz);
  s.bound = s.rows.staged ? 0 : gclim_bound(np);
  s.rpw = s.bound == GCLIM_NGMAX ? gclim_lds_rows(ng) : s.rows.rpb;
  s.nblk = (rows + s.rpw - 1) / s.rpw;
  s.lds_bytes = s.rows.staged ? (size_t)s.rows.rpb * (size_t)s.rows.stride * esz
                              : s.bound == GCLIM_NGMAX ? (size_t)s.rpw * (size_t)ng * 64 * 8 : 0;
  return s;
}

}  // namespace temx

#endif
