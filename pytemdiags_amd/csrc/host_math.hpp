// host_math.hpp -- host: the numbers behind a plan that need no device: Cholesky inverse and Jacobi pseudo-inverse of a
// Gram matrix, np.gradient tables, Gauss-Legendre quadrature and Y_l^0, the MFMA operand packing, and the matrices of
// the single sweep, of the missing-value mode and of the TEM pipeline that are assembled from them.  Arrays and sizes
// in, std::vectors out; no HIP, no plan, no environment.
#ifndef TEMX_HOST_MATH_HPP
#define TEMX_HOST_MATH_HPP
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

namespace temx {

// physical constants of the reference (PyTEMDiags/constants.py:6-14)
constexpr double kR = 287.058, kCp = 1004.64, kOm = 7.29212e-5;

// ---- Cholesky inverse of the K x K Gram matrix (K <= 64) ----------------------------------------------------------
// Li = L^-1 for G = L L^T (long double); -1 when G is not numerically positive definite
inline int spd_factor(const double* G, int K, std::vector<long double>& Li) {
  std::vector<long double> Lm((size_t)K * K, 0.0L);
  Li.assign((size_t)K * K, 0.0L);
  for (int i = 0; i < K; ++i) {
    for (int j = 0; j <= i; ++j) {
      long double s = G[i * K + j];
      for (int k = 0; k < j; ++k) s -= Lm[i * K + k] * Lm[j * K + k];
      if (i == j) {
        if (!(s > 0.0L) || !(s <= 1e300L)) return -1;
        Lm[i * K + i] = sqrtl(s);
      } else {
        Lm[i * K + j] = s / Lm[j * K + j];
      }
    }
  }
  // a rank-deficient Gram shows up as a tiny pivot relative to the diagonal
  for (int i = 0; i < K; ++i)
    if (Lm[i * K + i] * Lm[i * K + i] < 1e-13L * (long double)G[i * K + i]) return -1;
  for (int c = 0; c < K; ++c) {  // Li = L^-1 by forward substitution
    for (int i = c; i < K; ++i) {
      long double s = (i == c) ? 1.0L : 0.0L;
      for (int k = c; k < i; ++k) s -= Lm[i * K + k] * Li[k * K + c];
      Li[i * K + c] = s / Lm[i * K + i];
    }
  }
  return 0;
}

// G^-1 = L^-T L^-1
inline void inverse_from_factor(const std::vector<long double>& Li, int K, double* Ginv) {
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) {
      long double s = 0.0L;
      for (int k = std::max(i, j); k < K; ++k) s += Li[k * K + i] * Li[k * K + j];
      Ginv[i * K + j] = (double)s;
    }
}

// Pseudo-inverse of the symmetric positive semi-definite Gram matrix by cyclic Jacobi rotations
// (K <= 64).  Used when Cholesky fails: pinv(Y0) = pinv(G) Y0^T holds for any rank, which is the
// minimum-norm semantics of the reference's lstsq (gelsd) for a rank-deficient Y0 -- fewer distinct
// latitudes than harmonics.  Eigenvalues below 1e-12 * lambda_max are treated as zero.
inline int sym_pinv(const double* G, int K, double* Ginv, int* rank_out) {
  std::vector<long double> A((size_t)K * K), V((size_t)K * K, 0.0L);
  for (int i = 0; i < K * K; ++i) A[i] = G[i];
  for (int i = 0; i < K; ++i) V[(size_t)i * K + i] = 1.0L;
  for (int sweep = 0; sweep < 100; ++sweep) {
    long double off = 0.0L, diag = 0.0L;
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j) (i == j ? diag : off) += A[(size_t)i * K + j] * A[(size_t)i * K + j];
    if (off <= 1e-60L * diag) break;
    for (int p = 0; p < K - 1; ++p)
      for (int q = p + 1; q < K; ++q) {
        const long double apq = A[(size_t)p * K + q];
        if (apq == 0.0L) continue;
        const long double theta = (A[(size_t)q * K + q] - A[(size_t)p * K + p]) / (2.0L * apq);
        const long double t = (theta >= 0 ? 1.0L : -1.0L) / (fabsl(theta) + sqrtl(theta * theta + 1.0L));
        const long double c = 1.0L / sqrtl(t * t + 1.0L), sn = t * c;
        auto rot = [&](long double& a, long double& b) {   // (a, b) <- (c a - s b, s a + c b)
          const long double a0 = a, b0 = b;
          a = c * a0 - sn * b0;
          b = sn * a0 + c * b0;
        };
        for (int k = 0; k < K; ++k) rot(A[(size_t)k * K + p], A[(size_t)k * K + q]);   // A <- A J
        for (int k = 0; k < K; ++k) rot(A[(size_t)p * K + k], A[(size_t)q * K + k]);   // A <- J^T A
        for (int k = 0; k < K; ++k) rot(V[(size_t)k * K + p], V[(size_t)k * K + q]);   // V <- V J
      }
  }
  long double lmax = 0.0L;
  for (int i = 0; i < K; ++i) lmax = std::max(lmax, A[(size_t)i * K + i]);
  if (!(lmax > 0.0L)) return -1;
  int rank = 0;
  std::vector<long double> inv(K, 0.0L);
  for (int i = 0; i < K; ++i)
    if (A[(size_t)i * K + i] > 1e-12L * lmax) {
      inv[i] = 1.0L / A[(size_t)i * K + i];
      ++rank;
    }
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) {
      long double s2 = 0.0L;
      for (int k = 0; k < K; ++k) s2 += V[(size_t)i * K + k] * inv[k] * V[(size_t)j * K + k];
      Ginv[(size_t)i * K + j] = (double)s2;
    }
  *rank_out = rank;
  return 0;
}

// np.gradient(f, x) coefficient table out[i] = a f[i-1] + b f[i] + c f[i+1], edge_order = 1
// (tem_util.py:154, 192).  numpy switches to the uniform formula only when diff(x) is bit-uniform.
inline void gradient_table(const std::vector<double>& x, std::vector<double>& tab) {
  const int n = (int)x.size();
  tab.assign((size_t)n * 3, 0.0);
  std::vector<double> dx(n - 1);
  for (int i = 0; i + 1 < n; ++i) dx[i] = x[i + 1] - x[i];
  bool uniform = true;
  for (int i = 1; i + 1 < n; ++i) uniform = uniform && (dx[i] == dx[0]);
  for (int i = 1; i + 1 < n; ++i) {
    if (uniform) {
      tab[i * 3 + 0] = -1.0 / (2.0 * dx[0]);
      tab[i * 3 + 2] = 1.0 / (2.0 * dx[0]);
    } else {
      const double d1 = dx[i - 1], d2 = dx[i];
      tab[i * 3 + 0] = -(d2) / (d1 * (d1 + d2));
      tab[i * 3 + 1] = (d2 - d1) / (d1 * d2);
      tab[i * 3 + 2] = d1 / (d2 * (d1 + d2));
    }
  }
  tab[0 * 3 + 1] = -1.0 / dx[0];
  tab[0 * 3 + 2] = 1.0 / dx[0];
  tab[(n - 1) * 3 + 0] = -1.0 / dx[n - 2];
  tab[(n - 1) * 3 + 1] = 1.0 / dx[n - 2];
}

// Gauss-Legendre nodes and weights on [-1, 1] (long double, Newton on P_n)
inline void gauss_legendre(int n, std::vector<long double>& x, std::vector<long double>& w) {
  x.assign(n, 0.0L);
  w.assign(n, 0.0L);
  const long double pi = 3.141592653589793238462643383279502884L;
  for (int i = 0; i < (n + 1) / 2; ++i) {
    long double z = cosl(pi * (i + 0.75L) / (n + 0.5L)), pp = 0.0L;
    for (int it = 0; it < 100; ++it) {
      long double p1 = 1.0L, p2 = 0.0L;
      for (int j = 1; j <= n; ++j) {
        const long double p3 = p2;
        p2 = p1;
        p1 = ((2.0L * j - 1.0L) * z * p2 - (j - 1.0L) * p3) / j;
      }
      pp = n * (z * p1 - p2) / (z * z - 1.0L);
      const long double dz = p1 / pp;
      z -= dz;
      if (fabsl(dz) < 1e-19L) break;
    }
    x[i] = -z;
    x[n - 1 - i] = z;
    w[i] = w[n - 1 - i] = 2.0L / ((1.0L - z * z) * pp * pp);
  }
}

// normalised Y_l^0 at x = cos(colat), l < n (long double)
inline void ylm0_row(long double xv, int n, long double* y) {
  const long double pi = 3.141592653589793238462643383279502884L;
  long double pm1 = 1.0L, pc = xv;
  for (int l = 0; l < n; ++l) {
    long double P;
    if (l == 0) {
      P = 1.0L;
    } else if (l == 1) {
      P = xv;
    } else {
      const long double pn = ((2 * l - 1) * xv * pc - (l - 1) * pm1) / l;
      pm1 = pc;
      pc = pn;
      P = pn;
    }
    y[l] = sqrtl((2.0L * l + 1.0L) / (4.0L * pi)) * P;
  }
}

// ---- MFMA operand packing -----------------------------------------------------------------------------------------
// 4x4 MFMA A-operand blocks of a row-major R x K matrix: blk[rb][t][k*4+i] = A[4rb+i][4t+k], zero padded
inline std::vector<double> pack_blocks4(const double* A, int R, int K, int TB) {
  const int nrb = (R + 3) / 4;
  std::vector<double> blk((size_t)nrb * TB * 16, 0.0);
  for (int rb = 0; rb < nrb; ++rb)
    for (int t = 0; t < TB; ++t)
      for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * rb + i, col = 4 * t + k;
          if (r < R && col < K) blk[((size_t)rb * TB + t) * 16 + k * 4 + i] = A[(size_t)r * K + col];
        }
  return blk;
}

// 16 x 4 A-operand blocks (kernels_osc.hpp) of the R x C matrix A (row-major, leading dimension ld): nrb4 blocks of 4
// rows are padded to whole 16-row blocks, the columns to nkb blocks of 4; zero filled; appended to `out`
inline void append_blocks16(std::vector<double>& out, const double* A, int R, int C, int ld, bool transpose, int nrb4, int nkb) {
  const size_t o = out.size();
  const int nrb = (nrb4 + 3) / 4;
  out.resize(o + (size_t)nrb * nkb * 64, 0.0);
  for (int rb = 0; rb < nrb; ++rb)
    for (int t = 0; t < nkb; ++t)
      for (int k = 0; k < 4; ++k)
        for (int m = 0; m < 16; ++m) {
          const int r = 16 * rb + m, c = 4 * t + k;         // element [r][c] of the (transposed) matrix
          if (r < R && c < C) out[o + ((size_t)rb * nkb + t) * 64 + k * 16 + m] = transpose ? A[(size_t)c * ld + r] : A[(size_t)r * ld + c];
        }
}

// ---- quadrature basis ---------------------------------------------------------------------------------------------
// Y[q][l] = Y_l^0 at the q-th of nq Gauss-Legendre nodes, l < n, and w2[q] = 2 pi w_q: sum_q w2[q] f(x_q) is the
// integral over the sphere of a zonally symmetric f, exact to degree 2 nq - 1
struct QuadBasis {
  std::vector<long double> Y, w2;
};
inline QuadBasis quadrature_basis(int nq, int n) {
  QuadBasis qb;
  std::vector<long double> xq, wq;
  gauss_legendre(nq, xq, wq);
  qb.Y.resize((size_t)nq * n);
  qb.w2.resize((size_t)nq);
  const long double twopi = 6.283185307179586476925286766559005768L;
  for (int q = 0; q < nq; ++q) {
    ylm0_row(xq[(size_t)q], n, &qb.Y[(size_t)q * n]);
    qb.w2[(size_t)q] = twopi * wq[(size_t)q];
  }
  return qb;
}

// ---- single sweep (kernels_op2.hpp, kernels_osc.hpp): Gram matrices over the latitude classes ---------------------
// xc[4 * groups] cos(colat) of the classes and cnt[groups][2 sides][4] their member counts: ClassTables
// (class_tables.hpp).  Gram matrix [KR][KR] of the degrees < KR over the members of every S-th class-group.
inline std::vector<double> subsample_gram(const std::vector<double>& xc, const std::vector<double>& cnt, int64_t ngroups, int64_t S, int KR) {
  std::vector<long double> y((size_t)KR), Gl((size_t)KR * KR, 0.0L);
  for (int64_t gi = 0; gi < ngroups; gi += S)
    for (int k = 0; k < 4; ++k) {
      const long double nN = cnt[(size_t)gi * 8 + k], nS = cnt[(size_t)gi * 8 + 4 + k];
      if (nN + nS == 0.0L) continue;
      ylm0_row((long double)xc[(size_t)gi * 4 + k], KR, y.data());
      for (int l = 0; l < KR; ++l)
        for (int m = 0; m < KR; ++m) Gl[(size_t)l * KR + m] += (nN + (((l + m) & 1) ? -nS : nS)) * y[l] * y[m];
    }
  return std::vector<double>(Gl.begin(), Gl.end());
}

// Gx[l][k] = sum over the native columns of Y_l Y_k, l < K, k < KX, summed per latitude class in `nstripes` stripes
// (class ci belongs to stripe ci % nstripes), one host thread per stripe.  The partial sums stay per stripe and are
// added in stripe order, so the result has the same bits however the stripes were run.
inline std::vector<double> extended_gram(const std::vector<double>& xc, const std::vector<double>& cnt, int64_t ncls, int K, int KX, int nstripes) {
  const int nth = nstripes;
  std::vector<std::vector<double>> part((size_t)nth, std::vector<double>((size_t)K * KX, 0.0));
  std::vector<std::thread> th;
  auto stripe = [&](int t) {
    std::vector<double> yy((size_t)KX);
    std::vector<long double> y((size_t)KX);
    std::vector<double>& Gp = part[(size_t)t];
    for (int64_t ci = t; ci < ncls; ci += nth) {
      const int64_t gi = ci >> 2;
      const int k4 = (int)(ci & 3);
      const double nN = cnt[(size_t)gi * 8 + k4], nS = cnt[(size_t)gi * 8 + 4 + k4];
      ylm0_row((long double)xc[(size_t)ci], KX, y.data());
      for (int k = 0; k < KX; ++k) yy[(size_t)k] = (double)y[(size_t)k];
      const double se = nN + nS, so = nN - nS;
      for (int l = 0; l < K; ++l) {
        const double yl = yy[(size_t)l];
        double* row = &Gp[(size_t)l * KX];
        for (int k = (l & 1); k < KX; k += 2) row[k] += se * yl * yy[(size_t)k];        // l + k even
        for (int k = 1 - (l & 1); k < KX; k += 2) row[k] += so * yl * yy[(size_t)k];    // l + k odd
      }
    }
  };
  // a thread that cannot be started (std::system_error under a process / thread limit -- the callers are extern "C"
  // call chains, nothing may propagate) leaves its stripe to the caller
  int started = 0;
  try {
    th.reserve((size_t)nth);
    for (; started < nth - 1; ++started) th.emplace_back(stripe, started);
  } catch (...) {
  }
  for (int t = started; t < nth; ++t) stripe(t);
  for (auto& x : th) x.join();
  std::vector<double> Gx((size_t)K * KX, 0.0);
  for (int t = 0; t < nth; ++t)
    for (size_t i = 0; i < Gx.size(); ++i) Gx[i] += part[(size_t)t][i];
  return Gx;
}

// ---- missing-value mode (kernels_miss.hpp): tables of the per-d systems -------------------------------------------
// G2 [K][K] (as given), Zq [NQ][K], Yq [NQ][NE], Acov [K][K], c1 [K] with NE = NQ = 2L + 1.  G2 = Q^T Q over the
// plan's rows, T the upper triangular map from Y0 to the basis Q (the identity when the plan keeps Y0), Gi the
// operator coefficients = Gi Q^T a, x[N] = cos(colat) of the native columns.
inline std::vector<double> miss_tables(const double* G2, const double* T, const double* Gi, const double* x, int64_t N, int K, int L) {
  const int NE = 2 * L + 1, NQ = 2 * L + 1;
  std::vector<long double> s(K, 0.0L), y(K);          // s = Y0^T 1 (raw), from the latitudes
  for (int64_t i = 0; i < N; ++i) {
    ylm0_row(x[i], K, y.data());
    for (int l = 0; l < K; ++l) s[l] += y[l];
  }
  std::vector<double> tab(G2, G2 + (size_t)K * K);
  tab.reserve((size_t)2 * K * K + (size_t)NQ * (K + NE) + K);
  const QuadBasis qb = quadrature_basis(NQ, NE);
  for (int q = 0; q < NQ; ++q)                      // Zq[q][j] = sum_l Y_l(x_q) T[l][j]
    for (int j = 0; j < K; ++j) {
      long double a = 0.0L;
      for (int l = 0; l <= j; ++l) a += qb.Y[(size_t)q * NE + l] * T[(size_t)l * K + j];
      tab.push_back((double)a);
    }
  for (int q = 0; q < NQ; ++q)                      // Yq[q][n] = 2 pi w_q Y_n(x_q)
    for (int n = 0; n < NE; ++n) tab.push_back((double)(qb.w2[(size_t)q] * qb.Y[(size_t)q * NE + n]));
  std::vector<long double> sQ(K, 0.0L);            // Q^T 1 = T^T s
  for (int j = 0; j < K; ++j)
    for (int l = 0; l <= j; ++l) sQ[j] += s[l] * T[(size_t)l * K + j];
  for (int j = 0; j < K; ++j)                       // Acov = Gi T^T
    for (int l = 0; l < K; ++l) {
      long double a = 0.0L;
      for (int k = 0; k < K; ++k) a += (long double)Gi[(size_t)j * K + k] * T[(size_t)l * K + k];
      tab.push_back((double)a);
    }
  for (int j = 0; j < K; ++j) {                     // c1 = Gi Q^T 1
    long double a = 0.0L;
    for (int k = 0; k < K; ++k) a += (long double)Gi[(size_t)j * K + k] * sQ[k];
    tab.push_back((double)a);
  }
  return tab;
}

// ---- TEM pipeline: tables of the pressure levels p [Pa, ascending] and of the output latitudes [degrees] -----------
struct TemTables {
  std::vector<double> pg, lg;            // gradient_table of p and of the latitudes in radians
  std::vector<double> coslat, fcor;      // [M] cos(lat), Coriolis parameter
  std::vector<double> colscale;          // [nlev][nt] (p0 / p)^(R / Cp): theta = T colscale
};
inline TemTables tem_tables(const std::vector<double>& p, int64_t nt, double p0, const std::vector<double>& lat_deg) {
  TemTables tt;
  gradient_table(p, tt.pg);
  // f and cos(lat) use lat*pi/180 (tem_diagnostics.py:401-402), the gradient uses np.deg2rad(lat) = lat*(pi/180) (:586)
  const size_t M = lat_deg.size();
  std::vector<double> latr(M);
  tt.coslat.resize(M);
  tt.fcor.resize(M);
  for (size_t m = 0; m < M; ++m) {
    const double lat = lat_deg[m];
    latr[m] = lat * (M_PI / 180.0);
    tt.coslat[m] = std::cos(lat * M_PI / 180.0);
    tt.fcor[m] = 2 * kOm * std::sin(lat * M_PI / 180.0);
  }
  gradient_table(latr, tt.lg);
  // theta = T (p0/p)^k, k = R/Cp  (tem_diagnostics.py:498, constants.py:12): per-column scale
  tt.colscale.resize(p.size() * (size_t)nt);
  const double kap = kR / kCp;
  for (size_t j = 0; j < p.size(); ++j) {
    const double sc = std::pow(p0 / p[j], kap);
    for (int64_t t = 0; t < nt; ++t) tt.colscale[j * (size_t)nt + (size_t)t] = sc;
  }
  return tt;
}

}  // namespace temx

#endif
