// kernels_miss.hpp -- missing-value mode (TEMX_OPT_MISSING = 1): masked fits of fields with non-finite points.
//
// Per (level, time) column d the fit minimises  sum_{i valid} (a_i - f(x_i))^2 + tau sum_{i missing} f(x_i)^2  over
// f = sum_{l <= L} c_l Y_l^0.  In the plan's projection basis Q = Y0 T (T = R^-1 after temx_plan_finalize, the
// identity otherwise) the normal equations are H_d c = b_d with
//   b_d = Q^T (m_d ? a : 0)                        (a SELECT: NaN * 0 is NaN)
//   H_d = Q^T Q - (1 - tau) T^T G^miss_d T,  G^miss_d[l][l'] = sum_{i missing} Y_l Y_l'
// and G^miss_d follows from e_d[n] = sum_{i missing} Y_n(x_i), n <= 2L, by the Legendre product linearisation:
//   G^miss_d = sum_q what_q y(x_q) y(x_q)^T,  what_q = 2 pi w_q sum_n Y_n(x_q) e_d[n]   (NQ = 2L+1 Gauss nodes, exact).
// Kernels:
//   miss_basis_kernel    raw rows Y_n(x_i), n < 4 TBE, as 4x4 MFMA A blocks (the e projection; built once per plan)
//   miss_project_kernel  one read of the NF fields: common mask, select, theta scale, b (NF x K) and e (2L+1) sums
//   miss_system_kernel   per d: H_d, Cholesky in LDS, NR right-hand sides, coverage, zonal values with NaN
//   miss_native_kernel   native reconstruction of one field (temx_zonal_mean native = 1), NaN where missing / thin
//   miss_eddy_native_kernel  the seven native eddy fields of the TEM run, NaN where missing / thin
// The masked products of the eddy sweep are the KIND = 2 instantiation of eddy_kernel (kernels.hpp).
#pragma once
#include "kernels.hpp"

namespace temx {

constexpr int MISS_KMAX = 64;     // K <= 64 (L <= 63)
constexpr int MISS_NEMAX = 128;   // 2L + 1 <= 127 raw harmonics of the missing indicator

// raw rows up to n < 4 TBE (zero for n >= NE and for padding rows), blocked like yblk: eblk[group][t][k*4+i] = Y[4g+k][4t+i]
__global__ void miss_basis_kernel(const double* __restrict__ x, int64_t N, int64_t nrow_pad, int NE, int TBE,
                                  double* __restrict__ eblk) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nrow_pad) return;
  const bool valid = i < N;
  const double xv = valid ? x[i] : 0.0;
  const int64_t group = i >> 2;
  const int k = (int)(i & 3);
  double pm1 = 1.0, pc = xv;
  for (int l = 0; l < 4 * TBE; ++l) {
    double P;
    if (l == 0) {
      P = 1.0;
    } else if (l == 1) {
      P = xv;
    } else {
      const double pn = ((2 * l - 1) * xv * pc - (l - 1) * pm1) / l;
      pm1 = pc;
      pc = pn;
      P = pn;
    }
    const double val = (valid && l < NE) ? sqrt((2.0 * l + 1.0) / (4.0 * M_PI)) * P : 0.0;
    eblk[((group * TBE + (l >> 2)) * 16) + k * 4 + (l & 3)] = val;
  }
}

// partial[split][r][d], r < NF K: the select-projections of the fields on Q (field-major), then NE rows of the
// projection of the missing indicator on raw harmonics.  Tiling of project_kernel: one wave = one d-tile (16 columns),
// four waves per workgroup, the A blocks of a chunk (16 rows) staged in LDS once for all four.  A point is missing
// when any of the NF fields is not finite there; padding rows (>= N) are neither valid nor missing.
template <typename T, int NF, int TB, int TBE>
__global__ void __launch_bounds__(256)
miss_project_kernel(FieldPtrs<NF> fp, int64_t N, int64_t D, int K, int NE, const double* __restrict__ yblk, int gstride,
                    const double* __restrict__ eblk, int64_t nchunk, const double* __restrict__ colscale, int sfield,
                    double* __restrict__ partial, int nsplit, int ndt) {
  constexpr int YA = 4 * TB * 16, EA = 4 * TBE * 16;   // doubles of A blocks per chunk
  __shared__ double ystage[YA + EA];
  int split, dq;
  if (!wg_work((ndt + 3) / 4, nsplit, split, dq)) return;
  const int wave = uniform_wave();
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int dt = dq * 4 + wave;
  const bool active = dt < ndt;
  const int64_t d = (int64_t)dt * 16 + c;
  const bool dvalid = active && d < D;
  const int64_t dcl = d < D ? d : D - 1;
  const int64_t c0 = nchunk * split / nsplit, c1 = nchunk * (split + 1) / nsplit;
  const uint32_t yoff = (uint32_t)(g * 4 + (lane & 3));
  double sc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) sc[f] = (colscale != nullptr && f == sfield) ? colscale[dcl] : 1.0;

  double acc[NF][TB], acce[TBE];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int t = 0; t < TB; ++t) acc[f][t] = 0.0;
#pragma unroll
  for (int t = 0; t < TBE; ++t) acce[t] = 0.0;

  for (int64_t chunk = c0; chunk < c1; ++chunk) {
    // this lane's four rows of the chunk (issued before the staging so that their latency overlaps it)
    T xv[NF][4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
      int64_t row = chunk * 16 + ti * 4 + g;
      row = row < N ? row : N - 1;
#pragma unroll
      for (int f = 0; f < NF; ++f) xv[f][ti] = reinterpret_cast<const T*>(fp.p[f])[row * D + dcl];
    }
    __syncthreads();   // the previous chunk's blocks are no longer read
    for (int j = tid; j < YA; j += 256) {
      const int gi = j / (TB * 16), rem = j % (TB * 16);
      ystage[j] = yblk[((chunk * 4 + gi) * gstride) * 16 + rem];
    }
    for (int j = tid; j < EA; j += 256) ystage[YA + j] = eblk[chunk * EA + j];
    __syncthreads();
    if (active) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        const bool inrow = chunk * 16 + ti * 4 + g < N;
        bool ok = true;
        double xs[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          xs[f] = (double)xv[f][ti];
          ok = ok && isfinite(xs[f]);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) xs[f] = (ok && inrow) ? xs[f] * sc[f] : 0.0;
        const double miss = (!ok && inrow) ? 1.0 : 0.0;
#pragma unroll
        for (int t = 0; t < TB; ++t) {
          const double ya = ystage[(ti * TB + t) * 16 + yoff];
#pragma unroll
          for (int f = 0; f < NF; ++f) acc[f][t] = TEMX_MFMA4(ya, xs[f], acc[f][t]);
        }
#pragma unroll
        for (int t = 0; t < TBE; ++t) acce[t] = TEMX_MFMA4(ystage[YA + (ti * TBE + t) * 16 + yoff], miss, acce[t]);
      }
    }
  }
  if (dvalid) {
    const int64_t R = (int64_t)NF * K + NE;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int t = 0; t < TB; ++t) {
        const int l = t * 4 + g;
        if (l < K) partial[((int64_t)split * R + f * K + l) * D + d] = acc[f][t];
      }
#pragma unroll
    for (int t = 0; t < TBE; ++t) {
      const int n = t * 4 + g;
      if (n < NE) partial[((int64_t)split * R + NF * K + n) * D + d] = acce[t];
    }
  }
}

// Tables of the per-d systems (built on the host, host_math.hpp miss_tables).
struct MissTables {
  const double* G2;     // [K][K]   Q^T Q
  const double* Zq;     // [NQ][K]  Q-basis rows at the Gauss nodes: Zq[q][j] = sum_l Y_l(x_q) T[l][j]
  const double* Yq;     // [NQ][NE] 2 pi w_q Y_n(x_q)
  const double* Acov;   // [K][K]   Ginv T^T: coverage coefficients = c1 - Acov e[0..K)
  const double* c1;     // [K]      Ginv Q^T 1
  const double* Qp;     // [M][K]   Q-basis rows at the output latitudes
};

// One workgroup per column d.  Bf: [NR][K][D] select-projections; E: [NE][D] (projection of the missing indicator).
// Writes C ([NR][K4][D], rows >= K zero) and Ccov ([K4][D]) when not NULL, the zonal values zout [NR][M][D]
// (NaN where coverage < thr, thr > 0, or where the system did not factor) and the coverage [M][D] when not NULL.
template <int NR>
__global__ void __launch_bounds__(256)
miss_system_kernel(const double* __restrict__ Bf, const double* __restrict__ E, int K, int K4, int NE, int NQ, int M,
                   int64_t D, MissTables tb, double omt /* 1 - tau */, double thr, double* __restrict__ C,
                   double* __restrict__ Ccov, double* __restrict__ zout, double* __restrict__ cov_out) {
  __shared__ double H[MISS_KMAX][MISS_KMAX + 1];
  __shared__ double se[MISS_NEMAX], wh[MISS_NEMAX], cf[NR][MISS_KMAX], cc[MISS_KMAX];
  __shared__ int bad;
  const int64_t d = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) bad = 0;
  for (int n = tid; n < NE; n += 256) se[n] = E[(int64_t)n * D + d];
  __syncthreads();
  // weights of the Gauss nodes: the missing indicator synthesised from its degree-2L projection
  for (int q = tid; q < NQ; q += 256) {
    const double* yq = tb.Yq + (int64_t)q * NE;
    double a0 = 0.0, a1 = 0.0;
    int n = 0;
    for (; n + 1 < NE; n += 2) {
      a0 += yq[n] * se[n];
      a1 += yq[n + 1] * se[n + 1];
    }
    if (n < NE) a0 += yq[n] * se[n];
    wh[q] = a0 + a1;
  }
  // coverage coefficients (the default operator applied to the validity indicator)
  for (int j = tid; j < K; j += 256) {
    double a = tb.c1[j];
    for (int l = 0; l < K; ++l) a -= tb.Acov[(int64_t)j * K + l] * se[l];
    cc[j] = a;
  }
  __syncthreads();
  // lower triangle of H = G2 - (1 - tau) sum_q wh_q z_q z_q^T
  for (int idx = tid; idx < K * K; idx += 256) {
    const int i = idx / K, j = idx - i * K;
    if (j > i) continue;
    double a0 = 0.0, a1 = 0.0;
    int q = 0;
    for (; q + 1 < NQ; q += 2) {
      a0 += wh[q] * tb.Zq[(int64_t)q * K + i] * tb.Zq[(int64_t)q * K + j];
      a1 += wh[q + 1] * tb.Zq[(int64_t)(q + 1) * K + i] * tb.Zq[(int64_t)(q + 1) * K + j];
    }
    if (q < NQ) a0 += wh[q] * tb.Zq[(int64_t)q * K + i] * tb.Zq[(int64_t)q * K + j];
    H[i][j] = tb.G2[(int64_t)i * K + j] - omt * (a0 + a1);
  }
  // Cholesky H = L L^T in place (lower triangle), right looking
  for (int k = 0; k < K; ++k) {
    __syncthreads();
    const double dkk = H[k][k];
    const double lkk = sqrt(dkk);
    __syncthreads();
    if (tid == 0) {
      H[k][k] = lkk;
      if (!(dkk > 0.0) || !isfinite(dkk)) bad = 1;
    }
    for (int i = k + 1 + tid; i < K; i += 256) H[i][k] /= lkk;
    __syncthreads();
    const int nt = K - 1 - k;     // trailing block (k, K) x (k, K), lower triangle
    for (int idx = tid; idx < nt * nt; idx += 256) {
      const int i = k + 1 + idx / nt, j = k + 1 + idx % nt;
      if (j <= i) H[i][j] -= H[i][k] * H[j][k];
    }
  }
  __syncthreads();
  // one wave per right-hand side: forward and back substitution with the lanes along the rows
  if (wave < NR) {
    double y = lane < K ? Bf[((int64_t)wave * K + lane) * D + d] : 0.0;
    for (int k = 0; k < K; ++k) {
      if (lane == k) y /= H[k][k];
      const double yk = __shfl(y, k, 64);
      if (lane > k && lane < K) y -= H[lane][k] * yk;
    }
    for (int k = K - 1; k >= 0; --k) {
      if (lane == k) y /= H[k][k];
      const double yk = __shfl(y, k, 64);
      if (lane < k) y -= H[k][lane] * yk;
    }
    if (lane < K) cf[wave][lane] = y;
  }
  __syncthreads();
  const bool failed = bad != 0;
  const double qnan = __builtin_nan("");
  if (C != nullptr)
    for (int idx = tid; idx < NR * K4; idx += 256) {
      const int r = idx / K4, j = idx - r * K4;
      C[((int64_t)r * K4 + j) * D + d] = j < K ? (failed ? qnan : cf[r][j]) : 0.0;
    }
  if (Ccov != nullptr)
    for (int j = tid; j < K4; j += 256) Ccov[(int64_t)j * D + d] = j < K ? cc[j] : 0.0;
  for (int m = tid; m < M; m += 256) {
    const double* yp = tb.Qp + (int64_t)m * K;
    double cv = 0.0, v[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) v[r] = 0.0;
    for (int k = 0; k < K; ++k) {
      const double y = yp[k];
      cv += y * cc[k];
#pragma unroll
      for (int r = 0; r < NR; ++r) v[r] += y * cf[r][k];
    }
    const bool drop = failed || (thr > 0.0 && !(cv >= thr));
#pragma unroll
    for (int r = 0; r < NR; ++r) zout[((int64_t)r * M + m) * D + d] = drop ? qnan : v[r];
    if (cov_out != nullptr) cov_out[(int64_t)m * D + d] = cv;
  }
}

// Q[row][l] from the blocked copy (K <= 64: gstride == TB)
__device__ __forceinline__ double miss_q(const double* __restrict__ yblk, int gstride, int64_t row, int l) {
  return yblk[(((row >> 2) * gstride + (l >> 2)) * 16) + (row & 3) * 4 + (l & 3)];
}

// out[i][d] = Q[i] . C[:, d], NaN where x[i][d] is not finite or the native coverage Q[i] . Ccov[:, d] < thr
template <typename T>
__global__ void __launch_bounds__(256)
miss_native_kernel(const T* __restrict__ x, int64_t N, int64_t D, int K, const double* __restrict__ yblk, int gstride,
                   const double* __restrict__ C, const double* __restrict__ Ccov, double thr, double* __restrict__ out) {
  const int64_t total = N * D;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / D, d = idx - i * D;
    double v = 0.0, cv = 0.0;
    for (int l = 0; l < K; ++l) {
      const double q = miss_q(yblk, gstride, i, l);
      v += q * C[(int64_t)l * D + d];
      cv += q * Ccov[(int64_t)l * D + d];
    }
    const bool ok = isfinite((double)x[idx]) && !(thr > 0.0 && !(cv >= thr));
    out[idx] = ok ? v : __builtin_nan("");
  }
}

// The seven native eddy fields (tem_diagnostics.py:517-529, 547-555) for the rows [row0, row0 + nrows), written
// compactly ([nrows][D]); C: [4][K4][D] masked coefficients, Ccov: [K4][D].  NaN where any of the four fields is not
// finite or the native coverage is below thr.
template <typename T>
__global__ void __launch_bounds__(256)
miss_eddy_native_kernel(FieldPtrs<4> fp, int64_t row0, int64_t nrows, int64_t D, int K, int K4,
                        const double* __restrict__ yblk, int gstride, const double* __restrict__ C,
                        const double* __restrict__ Ccov, const double* __restrict__ colscale, double thr, EddyOut eo) {
  const int64_t total = nrows * D;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = idx / D, d = idx - r * D, i = row0 + r;
    double rec[4] = {0.0, 0.0, 0.0, 0.0}, cv = 0.0;
    for (int l = 0; l < K; ++l) {
      const double q = miss_q(yblk, gstride, i, l);
#pragma unroll
      for (int f = 0; f < 4; ++f) rec[f] += q * C[((int64_t)f * K4 + l) * D + d];
      cv += q * Ccov[(int64_t)l * D + d];
    }
    double x[4];
    bool ok = !(thr > 0.0 && !(cv >= thr));
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      x[f] = (double)reinterpret_cast<const T*>(fp.p[f])[i * D + d];
      ok = ok && isfinite(x[f]);
    }
    x[2] *= colscale[d];
    const double qnan = __builtin_nan("");
    double e[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) e[f] = ok ? x[f] - rec[f] : qnan;
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if (eo.p[f]) eo.p[f][idx] = e[f];
    if (eo.p[4]) eo.p[4][idx] = e[0] * e[1];
    if (eo.p[5]) eo.p[5][idx] = e[0] * e[3];
    if (eo.p[6]) eo.p[6][idx] = e[1] * e[2];
  }
}

}  // namespace temx
