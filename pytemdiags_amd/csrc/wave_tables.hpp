// wave_tables.hpp -- host: the tables of the zonal-wavenumber fit (kernels_wave.hpp, pytemdiags_amd/include/temx_wave.h).
// Pure functions of (L, m), the longitudes and small dense matrices; no HIP.
//
// A zonal wavenumber m in 1..L is fitted on the Kc = 2 (L + 1 - m) columns
//     Pbar_l^m(sin lat) cos(m lon),  Pbar_l^m(sin lat) sin(m lon),     l = m .. L   (cos half first),
// Pbar_l^m = sqrt(2) sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) P_l^m with the Condon-Shortley phase, computed by the normalised
// three-term recurrence (wave_pbar_row; no factorials, no overflow up to l = 511).  The basis is stored as 4x4 MFMA
// A-operand blocks, WAVE_SLICE_TB blocks (128 columns) per sweep: wave_shape gives the blocks per group and the
// instantiation of the last slice.  The Gram matrix Ym^T Ym is factorised here (wave_cholesky) and inverted from its
// factor.  tests/host/wave_tables_main.cpp runs this header on its own.
#ifndef TEMX_WAVE_TABLES_HPP
#define TEMX_WAVE_TABLES_HPP
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "dispatch.hpp"

namespace temx {

constexpr int WAVE_KC_MAX = 512;      // columns of one wavenumber's basis the solve serves
constexpr int WAVE_NM_MAX = 64;       // wavenumbers of one wave state
constexpr int WAVE_NF_MAX = 8;        // fields of one temxk_wave_project
constexpr int WAVE_SLICE_TB = 32;     // 4x4 blocks of basis columns one sweep keeps in accumulators (128 columns)
using WaveTBValues = IntList<4, 8, 16, 25, 32>;   // blocks per sweep the wave projection is instantiated for

inline int wave_ndeg(int L, int m) { return L + 1 - m; }
inline int wave_kc(int L, int m) { return 2 * wave_ndeg(L, m); }

// smallest instantiated number of blocks that holds nb (nb <= WAVE_SLICE_TB)
inline int wave_tb(int nb) { return nb <= 4 ? 4 : (nb <= 8 ? 8 : (nb <= 16 ? 16 : (nb <= 25 ? 25 : 32))); }

struct WaveShape {
  int ndeg = 0;      // degrees l = m .. L
  int Kc = 0;        // basis columns, 2 ndeg
  int nslice = 0;    // sweeps over the fields: ceil(blocks / WAVE_SLICE_TB)
  int tb_last = 0;   // blocks of the last sweep's instantiation
  int gstride = 0;   // blocks stored per group of 4 rows: WAVE_SLICE_TB (nslice - 1) + tb_last
  int kpad = 0;      // 4 gstride: columns of the blocked copy (columns >= Kc are zero)
};

inline WaveShape wave_shape(int L, int m) {
  WaveShape s;
  s.ndeg = wave_ndeg(L, m);
  s.Kc = 2 * s.ndeg;
  const int nb = (s.Kc + 3) / 4;
  s.nslice = (nb + WAVE_SLICE_TB - 1) / WAVE_SLICE_TB;
  s.tb_last = wave_tb(nb - WAVE_SLICE_TB * (s.nslice - 1));
  s.gstride = WAVE_SLICE_TB * (s.nslice - 1) + s.tb_last;
  s.kpad = 4 * s.gstride;
  return s;
}
// columns slice sl of the sweep produces, and the blocks of its instantiation
inline int wave_slice_cols(const WaveShape& s, int sl) {
  const int left = s.Kc - 4 * WAVE_SLICE_TB * sl;
  return left < 4 * WAVE_SLICE_TB ? left : 4 * WAVE_SLICE_TB;
}
inline int wave_slice_tb(const WaveShape& s, int sl) { return sl + 1 < s.nslice ? WAVE_SLICE_TB : s.tb_last; }

// out[l - m] = Pbar_l^m(x) for l = m .. L, x = sin(phi): a function of x alone, as scipy.special.lpmv(m, l, x) is, which
// the contract names.  cos(phi) is sqrt(1 - x^2), the form lpmv itself seeds its recurrence with, so the two agree to
// 2e-13 of a row's maximum at any latitude.  Next to a pole 1 - x^2 carries the rounding of x^2 (6e-12 of itself at 89.9
// degrees), m / 2 times over in cos^m(phi): against exact arithmetic in the same x a row there is off by 3e-12 (m = 1) to
// 9e-11 (m = 32) of its maximum, as lpmv is -- on values that are cos^m(phi) small beside the rows of other latitudes.
inline void wave_pbar_row(int m, int L, double x, double* out) {
  const double c = std::sqrt(1.0 - x * x);
  double r = (2.0 * m + 1.0) / (4.0 * M_PI);
  for (int k = 1; k <= m; ++k) r *= (2.0 * k - 1.0) / (2.0 * k);
  double cm = 1.0, cb = c;
  for (int e = m; e > 0; e >>= 1) {       // c^m by squaring, the multiplications of the device code (wave_pbar_each)
    if (e & 1) cm *= cb;
    cb *= cb;
  }
  double pmm = std::sqrt(2.0) * std::sqrt(r) * cm;
  if (m & 1) pmm = -pmm;
  out[0] = pmm;
  if (L == m) return;
  double p2 = pmm, p1 = std::sqrt(2.0 * m + 3.0) * x * pmm;
  out[1] = p1;
  for (int l = m + 2; l <= L; ++l) {
    const double l2 = (double)l * l, m2 = (double)m * m, q = (double)(l - 1) * (l - 1);
    const double a = std::sqrt((4.0 * l2 - 1.0) / (l2 - m2));
    const double b = std::sqrt((q - m2) / (4.0 * q - 1.0));
    const double p = a * (x * p1 - b * p2);
    p2 = p1;
    p1 = p;
    out[l - m] = p;
  }
}

// The arguments of temxk_wave_create that need no plan: 0, or the TEMX_E* code with the reason in msg.
inline int wave_check_args(int L, int64_t ncol, const double* lon_deg, int nm, const int* m, char* msg, size_t nmsg) {
  if (!lon_deg || !m) {
    snprintf(msg, nmsg, "null argument");
    return TEMX_EINVAL;
  }
  if (nm < 1 || nm > WAVE_NM_MAX) {
    snprintf(msg, nmsg, "nm must lie in 1..%d, got %d", WAVE_NM_MAX, nm);
    return TEMX_EINVAL;
  }
  for (int i = 0; i < nm; ++i) {
    if (m[i] < 1 || m[i] > L) {
      snprintf(msg, nmsg, "wavenumber %d is %d: a zonal wavenumber lies in 1..L = %d", i, m[i], L);
      return TEMX_EINVAL;
    }
    for (int j = 0; j < i; ++j)
      if (m[j] == m[i]) {
        snprintf(msg, nmsg, "wavenumber %d is given twice (entries %d and %d)", m[i], j, i);
        return TEMX_EINVAL;
      }
  }
  for (int64_t i = 0; i < ncol; ++i)
    if (!std::isfinite(lon_deg[i])) {
      snprintf(msg, nmsg, "lon %lld is not finite", (long long)i);
      return TEMX_EINVAL;
    }
  for (int i = 0; i < nm; ++i)
    if (wave_kc(L, m[i]) > WAVE_KC_MAX) {
      snprintf(msg, nmsg, "wavenumber %d at L = %d has Kc = %d basis columns: this version serves Kc <= %d", m[i], L,
               wave_kc(L, m[i]), WAVE_KC_MAX);
      return TEMX_EUNSUPPORTED;
    }
  return TEMX_OK;
}

// Cholesky factor of the symmetric matrix G [n][n] (row-major; the lower triangle is read): G = F F^T, F lower
// triangular, row-major in `F`.  0, or 1 + the first pivot that is refused.  The rank rule: a pivot is refused when it is
// at or below n 2^-52 max_j G[j][j] (or not finite).  A pivot that small lies inside the rounding of the Gram sums
// themselves, so its sign and size are noise: accepting it returns noise times its reciprocal as coefficients.  The
// measure is the LARGEST diagonal entry, not the pivot's own: a column the grid does not resolve (sin(m lon) at the
// Nyquist wavenumber of a lat-lon grid, 1e-16 everywhere) is orthogonal to the others, so its pivot is as large as its
// own diagonal entry, 1e-29 of the others.  The rule is relative: G times any positive factor is treated as G.  (With no
// positive diagonal entry the bound is 0 and the rule is "not positive".)
inline int wave_cholesky(const double* G, int n, std::vector<double>& F) {
  F.assign((size_t)n * n, 0.0);
  double dmax = 0.0;
  for (int j = 0; j < n; ++j)
    if (G[(size_t)j * n + j] > dmax) dmax = G[(size_t)j * n + j];
  const double least = (double)n * 0x1p-52 * dmax;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = G[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= F[(size_t)i * n + k] * F[(size_t)j * n + k];
      if (i == j) {
        if (!(s > least) || !std::isfinite(s)) return 1 + i;
        F[(size_t)i * n + i] = std::sqrt(s);
      } else {
        F[(size_t)i * n + j] = s / F[(size_t)j * n + j];
      }
    }
  return 0;
}

// Ginv [n][n] = (F F^T)^-1 from the factor: column by column, a forward and a back substitution
inline void wave_inverse_from_factor(const std::vector<double>& F, int n, double* Ginv) {
  std::vector<double> y((size_t)n);
  for (int c = 0; c < n; ++c) {
    for (int i = 0; i < n; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) s -= F[(size_t)i * n + k] * y[(size_t)k];
      y[(size_t)i] = s / F[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
      double s = y[(size_t)i];
      for (int k = i + 1; k < n; ++k) s -= F[(size_t)k * n + i] * Ginv[(size_t)k * n + c];
      Ginv[(size_t)i * n + c] = s / F[(size_t)i * n + i];
    }
  }
}

}  // namespace temx
#endif
