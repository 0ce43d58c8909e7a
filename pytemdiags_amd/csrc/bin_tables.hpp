// bin_tables.hpp -- host: the tables of the latitude-bin sweeps (kernels_bin.hpp, TEMX_OPT_LAT_BINS).  The latitude
// axis phi in [-pi/2, pi/2] is cut into B uniform bins of half-width h = pi / (2 B); inside a bin Y_l^0 is replaced by
// its Chebyshev interpolant of degree J - 1 in s = (phi - centre) / h,
//     Y_l(phi_i) ~ sum_{j<J} T_j(s_i) a[bin][j][l],        error <= 2 (l h / 2)^J / J!   (Bessel tail of cos(l phi)),
// so that a column contributes J local moments instead of K = L + 1 harmonics.  Here: the bound and the choice of J, the
// rows sorted by bin and cut into chunks, and the coefficient tables.  Arrays and sizes in, std::vectors out; no HIP, no
// plan, no environment.
#ifndef TEMX_BIN_TABLES_HPP
#define TEMX_BIN_TABLES_HPP
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_math.hpp"

namespace temx {

constexpr int BIN_ROWS = 512;        // R: most rows of one chunk (one wave walks a chunk for a window of 64 columns)
constexpr int BIN_DEFAULT = 512;     // B of TEMX_OPT_LAT_BINS = -1
constexpr int BIN_MAX_DEGREE = 12;   // largest J the kernels are instantiated for
constexpr double BIN_BOUND = 1e-13;  // what the interpolation error of a basis row may be

inline bool bin_count_ok(int B) { return B == 128 || B == 256 || B == 512 || B == 1024 || B == 2048; }

// 2 (L h / 2)^J / J!, h = pi / (2 B)
inline double bin_bound(int L, int B, int J) {
  const double a = 0.5 * L * (M_PI / (2.0 * B));
  double t = 2.0;
  for (int j = 1; j <= J; ++j) t *= a / j;
  return t;
}

// the smallest J of {8, 10, 12} that meets BIN_BOUND for degree L on B bins; 0: none does
inline int bin_degree(int L, int B) {
  for (int J = 8; J <= BIN_MAX_DEGREE; J += 2)
    if (bin_bound(L, B, J) <= BIN_BOUND) return J;
  return 0;
}

// inner and outer edges of the bins: edge(0) = -pi/2, edge(B) ~ pi/2
inline double bin_edge(int B, int i) { return -0.5 * M_PI + i * (M_PI / B); }

// bin of phi [rad]: a latitude on an inner edge belongs to the upper bin, +pi/2 (and anything beyond) to the last,
// anything below edge(1) to the first (np.searchsorted(inner edges, phi, side="right"))
inline int bin_index(double phi, int B) {
  int b = (int)std::floor((phi + 0.5 * M_PI) / (M_PI / B));
  b = std::max(0, std::min(B - 1, b));
  while (b + 1 <= B - 1 && phi >= bin_edge(B, b + 1)) ++b;
  while (b > 0 && phi < bin_edge(B, b)) --b;
  return b;
}

// local coordinate of phi in bin b, clamped to [-1, 1]
inline double bin_local(double phi, int B, int b) {
  const double h = M_PI / (2.0 * B), centre = -0.5 * M_PI + (b + 0.5) * (M_PI / B);
  return std::max(-1.0, std::min(1.0, (phi - centre) / h));
}

struct BinRows {
  int B = 0;
  std::vector<int> rows;        // [N] native rows, stably sorted by bin
  std::vector<double> s;        // [N] local coordinate of rows[i]
  std::vector<int> chunk;       // [nchunk][4]: bin, first sorted position, rows (1 .. BIN_ROWS), 0
  std::vector<int> bin_chunk0;  // [B + 1] first chunk of every bin (empty bins: an empty range)
  int64_t nchunk() const { return (int64_t)chunk.size() / 4; }
};

// false: a latitude is not finite or lies outside [-90, 90], or N does not fit the int row table
inline bool build_bin_rows(const double* lat_deg, int64_t N, int B, BinRows& out) {
  if (N < 1 || N >= ((int64_t)1 << 31) - 1 || B < 1) return false;
  out = BinRows();
  out.B = B;
  std::vector<int> bin((size_t)N);
  std::vector<int64_t> start((size_t)B + 1, 0);
  for (int64_t i = 0; i < N; ++i) {
    const double lat = lat_deg[i];
    if (!(lat >= -90.0 && lat <= 90.0)) return false;
    bin[(size_t)i] = bin_index(lat * (M_PI / 180.0), B);
    ++start[(size_t)bin[(size_t)i] + 1];
  }
  for (int b = 0; b < B; ++b) start[(size_t)b + 1] += start[(size_t)b];
  out.rows.resize((size_t)N);
  out.s.resize((size_t)N);
  std::vector<int64_t> fill(start.begin(), start.end() - 1);
  for (int64_t i = 0; i < N; ++i) {          // counting sort: rows of a bin keep their order
    const int b = bin[(size_t)i];
    const int64_t o = fill[(size_t)b]++;
    out.rows[(size_t)o] = (int)i;
    out.s[(size_t)o] = bin_local(lat_deg[i] * (M_PI / 180.0), B, b);
  }
  out.bin_chunk0.resize((size_t)B + 1);
  for (int b = 0; b < B; ++b) {
    out.bin_chunk0[(size_t)b] = (int)out.nchunk();
    for (int64_t o = start[(size_t)b]; o < start[(size_t)b + 1]; o += BIN_ROWS) {
      const int n = (int)std::min<int64_t>(BIN_ROWS, start[(size_t)b + 1] - o);
      out.chunk.insert(out.chunk.end(), {b, (int)o, n, 0});
    }
  }
  out.bin_chunk0[(size_t)B] = (int)out.nchunk();
  return true;
}

// a[B][J][KP]: Chebyshev coefficients of Y_l^0, l <= L, on every bin (columns L + 1 .. KP - 1 are zero).  Y_l at the J
// Chebyshev nodes of the bin in long double (ylm0_row at x = sin(phi)), then the J x J cosine transform.  Depends on
// (L, B, J) only.
inline std::vector<double> bin_coefficients(int L, int B, int J, int KP) {
  const int K = L + 1;
  const long double pi = 3.141592653589793238462643383279502884L;
  const long double h = pi / (2.0L * B);
  std::vector<double> a((size_t)B * J * KP, 0.0);
  std::vector<long double> y((size_t)J * K), ct((size_t)J * J);
  for (int j = 0; j < J; ++j)
    for (int m = 0; m < J; ++m) ct[(size_t)j * J + m] = cosl(pi * j * (m + 0.5L) / J);
  for (int b = 0; b < B; ++b) {
    const long double centre = -0.5L * pi + (b + 0.5L) * (pi / B);
    for (int m = 0; m < J; ++m) ylm0_row(sinl(centre + h * ct[(size_t)J + m]), K, &y[(size_t)m * K]);   // ct[1][m] = node m
    for (int j = 0; j < J; ++j)
      for (int l = 0; l < K; ++l) {
        long double c = 0.0L;
        for (int m = 0; m < J; ++m) c += y[(size_t)m * K + l] * ct[(size_t)j * J + m];
        a[((size_t)b * J + j) * KP + l] = (double)(c * (j == 0 ? 1.0L : 2.0L) / J);
      }
  }
  return a;
}

// sum_j T_j(s) a[bin][j][l], l < K: the interpolated basis row (tests; the kernels never form it)
inline void bin_row(const std::vector<double>& a, int J, int KP, int K, int bin, double s, double* y) {
  double t[BIN_MAX_DEGREE];
  t[0] = 1.0;
  t[1] = s;
  for (int j = 2; j < J; ++j) t[j] = 2.0 * s * t[j - 1] - t[j - 2];
  for (int l = 0; l < K; ++l) {
    double v = 0.0;
    for (int j = 0; j < J; ++j) v += t[j] * a[((size_t)bin * J + j) * KP + l];
    y[l] = v;
  }
}

}  // namespace temx

#endif
