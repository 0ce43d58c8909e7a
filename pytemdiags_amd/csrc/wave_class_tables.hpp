// wave_class_tables.hpp -- host: the tables of the class form of the zonal-wavenumber fit (kernels_wavecls.hpp,
// pytemdiags_amd/include_wavecls/temx_wavecls.h).  Arrays and sizes in, std::vectors out; no HIP, no plan, no environment.
//
// Columns of one class side (class_tables.hpp) share Pbar_l^m(sin lat) and their row of P Ym, P the plan's native
// zonal-mean operator, so per field and column d
//     (Ym - P Ym)^T x = sum_sides  Pbar(lat_s) (x) [ sum_i x_i cos(m lon_i), sum_i x_i sin(m lon_i) ]  -  Z_s sum_i x_i
// with Z_s [Kc] the row of P Ym on that side.  Pbar_l^m(-x) = (-1)^(l-m) Pbar_l^m(x): the even/odd split of the class
// basis ycls applies with the degree offset r = l - m in place of l.  What the sweep needs beside the plan's row table:
//   weights      {cos m lon, sin m lon} of every entry of crow (zero for padding entries and padding batches)
//   reps         one representative row per class and side (its first member): where Z_s is read
//   group table  per class-group, one run of 10 TBS 4x4 blocks: 2 TBS blocks of the class basis (TBS of even r, then TBS
//                of odd r; the layout of ycls), 4 TBS blocks of -E and 4 TBS of -O, E = (Z_N + Z_S) / 2,
//                O = (Z_N - Z_S) / 2 (cos half: even r, odd r; then the sin half), so that the deflation term is
//                -E (S0_N + S0_S) - O (S0_N - S0_S)
// tests/host/wave_class_tables_main.cpp runs this header on its own.
#ifndef TEMX_WAVE_CLASS_TABLES_HPP
#define TEMX_WAVE_CLASS_TABLES_HPP
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "class_tables.hpp"
#include "dispatch.hpp"
#include "shared_defs.hpp"

namespace temx {

constexpr int WAVECLS_NDEG_MAX = 64;            // degrees of one wavenumber the class form serves (TBS <= 8)
using WaveClsTBSValues = IntList<2, 4, 7, 8>;   // blocks per parity the class sweep is instantiated for
constexpr int WAVECLS_WPS = 2;                  // waves per SIMD of the class sweep
constexpr int WAVECLS_ROWMASK = CLS_HASPAD_BIT - 1;

// smallest instantiated number of blocks per parity that holds the even degree offsets of ndeg degrees
constexpr int wavecls_tbs(int ndeg) {
  const int b = ((ndeg + 1) / 2 + 3) / 4;
  return b <= 2 ? 2 : (b <= 4 ? 4 : (b <= 7 ? 7 : 8));
}

struct WaveClsShape {
  int ndeg = 0;    // degrees l = m .. L
  int Kc = 0;      // basis columns, 2 ndeg
  int TBS = 0;     // blocks per parity of the instantiation
  int nacc = 0;    // accumulators per field and lane: 4 TBS (cos even, cos odd, sin even, sin odd)
  int fpw = 1;     // fields per wave
};
inline WaveClsShape wavecls_shape(int L, int m) {
  WaveClsShape s;
  s.ndeg = L + 1 - m;
  s.Kc = 2 * s.ndeg;
  s.TBS = wavecls_tbs(s.ndeg);
  s.nacc = 4 * s.TBS;
  return s;
}

// ---- block layout of a class-group's table (doubles) -----------------------------------------------------------------
constexpr int wavecls_basis_doubles(int TBS) { return 2 * TBS * 16; }
constexpr int wavecls_defl_doubles(int TBS) { return 4 * TBS * 16; }
constexpr int wavecls_group_doubles(int TBS) { return wavecls_basis_doubles(TBS) + 2 * wavecls_defl_doubles(TBS); }
// class basis: Pbar of degree offset r = l - m at class k of the group
constexpr int wavecls_basis_slot(int TBS, int r, int k) {
  const int h = r >> 1;
  return ((r & 1) * TBS + (h >> 2)) * 16 + k * 4 + (h & 3);
}
// deflation tables: basis column j in [0, Kc) (cos half, then sin half) at class k; which = 0 for -E, 1 for -O
constexpr int wavecls_defl_slot(int TBS, int ndeg, int j, int k, int which) {
  const int half = j >= ndeg ? 1 : 0;
  return wavecls_basis_doubles(TBS) + which * wavecls_defl_doubles(TBS) + half * wavecls_basis_doubles(TBS) +
         wavecls_basis_slot(TBS, j - half * ndeg, k);
}
// the way back: basis column of element i of accumulator block a in [0, 4 TBS), -1 for padding
constexpr int wavecls_acc_col(int TBS, int ndeg, int a, int i) {
  const int half = a / (2 * TBS), t = a % (2 * TBS);
  const int r = t < TBS ? 2 * (4 * t + i) : 2 * (4 * (t - TBS) + i) + 1;
  return r < ndeg ? half * ndeg + r : -1;
}

// ---- per-entry weights, aligned with crow ----------------------------------------------------------------------------
// out[2 e], out[2 e + 1] = cos(m lon), sin(m lon) of the member row of entry e; zero for padding entries
inline std::vector<double> wavecls_weights(const std::vector<int>& crow, const double* lon_rad, int m) {
  std::vector<double> w(2 * crow.size(), 0.0);
  for (size_t e = 0; e < crow.size(); ++e) {
    if (crow[e] < 0) continue;
    const double a = (double)m * lon_rad[(size_t)(crow[e] & WAVECLS_ROWMASK)];
    w[2 * e] = std::cos(a);
    w[2 * e + 1] = std::sin(a);
  }
  return w;
}

// ---- one representative row per class and side ------------------------------------------------------------------------
// out[2 ci + side] for ci < 4 (ngroups + 1): the first member of that side in the row table, -1 for a side without members
inline std::vector<int> wavecls_representatives(const std::vector<int>& crow, const std::vector<int>& gbatch0, int64_t ngroups) {
  constexpr int MB = CLS_MB;
  std::vector<int> rep((size_t)(ngroups + 1) * 8, -1);
  for (int64_t gi = 0; gi < ngroups; ++gi)
    for (int b = gbatch0[(size_t)gi]; b < gbatch0[(size_t)gi + 1]; ++b)
      for (int k = 0; k < 4; ++k)
        for (int j = 0; j < MB; ++j) {
          const int ent = crow[((size_t)b * 4 + k) * MB + j];
          if (ent < 0) continue;
          int& r = rep[((size_t)gi * 4 + k) * 2 + ((ent >> 28) & CLS_SOUTH)];
          if (r < 0) r = ent & WAVECLS_ROWMASK;
        }
  return rep;
}

// ---- work cuts ----------------------------------------------------------------------------------------------------------
// how many of the nsub - 1 inner cuts of work_cuts (not group-aligned) fall inside a class-group
inline int wavecls_cuts_inside(const std::vector<int>& gbatch0, int64_t ngroups, int64_t nbatches, int nsub) {
  const std::vector<int> cut = work_cuts(gbatch0, ngroups, nbatches, nsub, false);
  int n = 0;
  for (int k = 1; k < nsub; ++k)
    if (cut[(size_t)2 * k] != gbatch0[(size_t)cut[(size_t)2 * k + 1]]) ++n;
  return n;
}

}  // namespace temx
#endif
