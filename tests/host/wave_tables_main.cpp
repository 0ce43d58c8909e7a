// The host tables of the zonal-wavenumber fit (pytemdiags_amd/csrc/wave_tables.hpp) on their own: the header needs no
// HIP.  usage: wave_tables_main
// Prints, for m in {1, 4, 32} and L = 255, at the latitudes of `lats`, one line "P m lat_index v_m v_{m+1} ... v_L" of
// Pbar_l^m(sin lat) (17 significant digits; tests/test_wave_host.py compares them with scipy), then checks on its own:
// the Kc / padding arithmetic of wave_shape for every (L, m) up to L = 511, the argument checker's codes, and the
// Cholesky factor and inverse on a small matrix, and the rank rule of wave_cholesky (a positive definite matrix with one
// row and column scaled by 1e-14 is refused at that pivot; the same matrix times 1e-30 overall is accepted; an accepted
// matrix keeps the textbook factor bit for bit).  Prints "shapes=<n> refusals=<n> cholesky=ok rank=ok"; a failed check
// prints the case and exits 1.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../pytemdiags_amd/csrc/wave_tables.hpp"

static int bad(const char* what, int a, int b) {
  std::printf("FAILED %s (%d, %d)\n", what, a, b);
  return 1;
}

int main() {
  using namespace temx;
  const double lats[] = {-89.9, -60.0, -23.5, 0.0, 10.0, 45.0, 75.0, 89.9};
  const int L = 255;
  for (int m : {1, 4, 32}) {
    std::vector<double> row((size_t)wave_ndeg(L, m));
    for (int j = 0; j < 8; ++j) {
      const double phi = lats[j] * M_PI / 180.0;
      wave_pbar_row(m, L, std::sin(phi), row.data());
      std::printf("P %d %d", m, j);
      for (double v : row) std::printf(" %.17g", v);
      std::printf("\n");
    }
  }
  // m = L: one degree
  {
    double one[1];
    wave_pbar_row(7, 7, 0.3, one);
    if (!(one[0] < 0.0)) return bad("Condon-Shortley sign of an odd m", 7, 7);
  }
  // ---- shapes ----
  long long shapes = 0;
  for (int Lq = 1; Lq <= 511; ++Lq)
    for (int m = 1; m <= Lq; ++m) {
      const WaveShape s = wave_shape(Lq, m);
      ++shapes;
      if (s.ndeg != Lq + 1 - m || s.Kc != 2 * s.ndeg || s.Kc != wave_kc(Lq, m)) return bad("Kc", Lq, m);
      if (s.kpad != 4 * s.gstride || s.kpad < s.Kc) return bad("padding holds the basis", Lq, m);
      if (s.nslice < 1 || s.gstride != WAVE_SLICE_TB * (s.nslice - 1) + s.tb_last) return bad("stride", Lq, m);
      if (s.tb_last != 4 && s.tb_last != 8 && s.tb_last != 16 && s.tb_last != 25 && s.tb_last != 32) return bad("instantiation", Lq, m);
      int cols = 0;
      for (int sl = 0; sl < s.nslice; ++sl) {
        const int c = wave_slice_cols(s, sl), tb = wave_slice_tb(s, sl);
        if (c < 1 || c > 4 * tb || tb > WAVE_SLICE_TB) return bad("slice columns fit its blocks", Lq, m);
        if (WAVE_SLICE_TB * sl + tb > s.gstride) return bad("slice stays inside a group's blocks", Lq, m);
        cols += c;
      }
      if (cols != s.Kc) return bad("slices cover the basis once", Lq, m);
      if (s.Kc <= 4 * WAVE_SLICE_TB && s.nslice != 1) return bad("one sweep up to 128 columns", Lq, m);
    }
  // ---- the checker ----
  int refusals = 0;
  char msg[256];
  const double lon[4] = {0.0, 90.0, 180.0, 270.0};
  const double lon_bad[4] = {0.0, std::numeric_limits<double>::quiet_NaN(), 180.0, 270.0};
  const double lon_inf[4] = {0.0, 90.0, std::numeric_limits<double>::infinity(), 270.0};
  const int m12[2] = {1, 2}, m0[1] = {0}, mbig[1] = {11}, mdup[3] = {2, 3, 2}, m1[1] = {1};
  auto expect = [&](int got, int want, const char* what) {
    if (got != want) {
      std::printf("FAILED checker %s: got %d, expected %d (%s)\n", what, got, want, msg);
      return false;
    }
    if (want != TEMX_OK) {
      ++refusals;
      if (msg[0] == 0) return false;
    }
    return true;
  };
  msg[0] = 0;
  if (!expect(wave_check_args(10, 4, lon, 2, m12, msg, sizeof msg), TEMX_OK, "good")) return 1;
  if (!expect(wave_check_args(10, 4, nullptr, 2, m12, msg, sizeof msg), TEMX_EINVAL, "null lon")) return 1;
  if (!expect(wave_check_args(10, 4, lon, 2, nullptr, msg, sizeof msg), TEMX_EINVAL, "null m")) return 1;
  if (!expect(wave_check_args(10, 4, lon, 0, m12, msg, sizeof msg), TEMX_EINVAL, "nm = 0")) return 1;
  if (!expect(wave_check_args(10, 4, lon, WAVE_NM_MAX + 1, m12, msg, sizeof msg), TEMX_EINVAL, "nm too large")) return 1;
  if (!expect(wave_check_args(10, 4, lon, 1, m0, msg, sizeof msg), TEMX_EINVAL, "m = 0")) return 1;
  if (!expect(wave_check_args(10, 4, lon, 1, mbig, msg, sizeof msg), TEMX_EINVAL, "m > L")) return 1;
  if (!expect(wave_check_args(10, 4, lon, 3, mdup, msg, sizeof msg), TEMX_EINVAL, "duplicate")) return 1;
  if (!expect(wave_check_args(10, 4, lon_bad, 2, m12, msg, sizeof msg), TEMX_EINVAL, "NaN lon")) return 1;
  if (!expect(wave_check_args(10, 4, lon_inf, 2, m12, msg, sizeof msg), TEMX_EINVAL, "infinite lon")) return 1;
  if (!expect(wave_check_args(257, 4, lon, 1, m1, msg, sizeof msg), TEMX_EUNSUPPORTED, "Kc = 514")) return 1;
  if (!expect(wave_check_args(256, 4, lon, 1, m1, msg, sizeof msg), TEMX_OK, "Kc = 512")) return 1;
  // ---- Cholesky and inverse ----
  {
    const int n = 5;
    std::vector<double> A((size_t)n * n), G((size_t)n * n, 0.0), F, Gi((size_t)n * n);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) A[(size_t)i * n + j] = std::sin(1.0 + 3.0 * i + 0.7 * j) + (i == j ? 2.0 : 0.0);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j)
        for (int k = 0; k < n; ++k) G[(size_t)i * n + j] += A[(size_t)k * n + i] * A[(size_t)k * n + j];
    if (wave_cholesky(G.data(), n, F) != 0) return bad("factor of a positive definite matrix", n, 0);
    wave_inverse_from_factor(F, n, Gi.data());
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += G[(size_t)i * n + k] * Gi[(size_t)k * n + j];
        if (std::fabs(s - (i == j ? 1.0 : 0.0)) > 1e-12) return bad("G Ginv = I", i, j);
      }
    // ---- the rank rule: a pivot at or below n 2^-52 max_j G[j][j] is refused ----
    // the factor of an accepted matrix is that of the textbook recurrence, bit for bit (the rule only refuses)
    auto textbook = [](const std::vector<double>& Gm, int nn) {
      std::vector<double> T((size_t)nn * nn, 0.0);
      for (int i = 0; i < nn; ++i)
        for (int j = 0; j <= i; ++j) {
          double s = Gm[(size_t)i * nn + j];
          for (int k = 0; k < j; ++k) s -= T[(size_t)i * nn + k] * T[(size_t)j * nn + k];
          T[(size_t)i * nn + j] = i == j ? std::sqrt(s) : s / T[(size_t)j * nn + j];
        }
      return T;
    };
    if (F != textbook(G, n)) return bad("the factor of an accepted matrix is unchanged", n, 0);
    // the same matrix times 1e-30 overall: accepted (the rule is relative), and its inverse is still one
    std::vector<double> Gs(G);
    for (double& v : Gs) v *= 1e-30;
    if (wave_cholesky(Gs.data(), n, F) != 0) return bad("a small but well-conditioned matrix is accepted", n, 0);
    if (F != textbook(Gs, n)) return bad("the factor of the scaled matrix is the textbook one", n, 0);
    wave_inverse_from_factor(F, n, Gi.data());
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += Gs[(size_t)i * n + k] * Gi[(size_t)k * n + j];
        if (std::fabs(s - (i == j ? 1.0 : 0.0)) > 1e-12) return bad("scaled G Ginv = I", i, j);
      }
    // one row and column scaled by 1e-14 (a basis column of 1e-14, its Gram entry 1e-28): still positive definite in
    // exact arithmetic, with a positive pivot -- refused, at that pivot, wherever it stands
    for (int r = 0; r < n; ++r) {
      std::vector<double> Gr(G);
      for (int k = 0; k < n; ++k) {
        Gr[(size_t)r * n + k] *= 1e-14;
        Gr[(size_t)k * n + r] *= 1e-14;
      }
      const std::vector<double> T = textbook(Gr, n);
      if (!(T[(size_t)r * n + r] > 0.0)) return bad("the scaled pivot is positive: the old rule accepted it", n, r);
      if (wave_cholesky(Gr.data(), n, F) != 1 + r) return bad("a pivot inside the rounding of the sums is refused, and named", n, r);
    }
    // just above the bound is accepted, at the bound is refused: diag(1, t), bound 2 * 2^-52
    {
      const double at = 2 * 0x1p-52;
      const double up[4] = {1.0, 0.0, 0.0, at * (1 + 0x1p-52)}, on[4] = {1.0, 0.0, 0.0, at};
      if (wave_cholesky(up, 2, F) != 0) return bad("a pivot above the bound is accepted", 2, 1);
      if (wave_cholesky(on, 2, F) != 2) return bad("a pivot at the bound is refused", 2, 1);
    }
    G[(size_t)3 * n + 3] = -1.0;
    if (wave_cholesky(G.data(), n, F) != 4) return bad("the failing pivot is named", n, 3);
    // no positive diagonal entry: the bound is 0, the first pivot fails
    const double neg[4] = {-1.0, 0.0, 0.0, -2.0}, zero[1] = {0.0};
    if (wave_cholesky(neg, 2, F) != 1 || wave_cholesky(zero, 1, F) != 1) return bad("no positive diagonal", 2, 0);
  }
  std::printf("shapes=%lld refusals=%d cholesky=ok rank=ok\n", shapes, refusals);
  return 0;
}
