// kernels_bin.hpp -- device: the latitude-bin form of the sweeps (TEMX_OPT_LAT_BINS; tables: bin_tables.hpp).
//
// Inside a latitude bin the basis row of a column is  Y_l(phi_i) = sum_{j<J} T_j(s_i) a[bin][j][l]  (T_j the Chebyshev
// polynomials of the column's local coordinate), so a projection  sum_i Y_l(phi_i) x_i  is a per-bin contraction of the
// J local moments  m[j] = sum_i T_j(s_i) x_i,  and a native zonal mean is a local Chebyshev series with the per-bin
// coefficients  z[j] = sum_l a[bin][j][l] c_l.  The two sweeps over the fields therefore cost J fused multiply-adds
// per field and grid point on the vector ALUs, with T_j(s_i) the same for all 64 lanes of a wave -- no matrix-core work
// of size K per column -- and everything of size K happens per bin.
//
// Work unit of the sweeps: one wave = one chunk (at most BIN_ROWS sorted rows of one bin) x one window of 64
// (lev, time) columns; loads are 1 row x 64 columns with a wave-uniform row address.  The four waves of
// a workgroup take four neighbouring windows of one chunk.  fp32 fields are widened on load, every sum is fp64.  Tails
// in D are masked: a lane beyond D loads nothing and contributes zeros.  All offsets are 64-bit.
//
// Every sum has a fixed order (rows of a chunk in sorted order, chunks of a bin in order, bins of a slab in order,
// slabs by reduce_partials): repeated runs give the same bits.
#ifndef TEMX_KERNELS_BIN_HPP
#define TEMX_KERNELS_BIN_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"

namespace temx {

constexpr int BIN_UNROLL = 4;       // rows whose loads are in flight together (x NF fields x 512 B per wave)
constexpr int BIN_SLABS = 16;       // slabs of bins the per-bin contraction is cut into (summed by reduce_partials)

// T_j(s), j < J, by the recurrence; s is wave-uniform
template <int J>
__device__ __forceinline__ void bin_cheb(double s, double (&t)[J]) {
  t[0] = 1.0;
  t[1] = s;
  const double s2 = s + s;
#pragma unroll
  for (int j = 2; j < J; ++j) t[j] = fma(s2, t[j - 1], -t[j - 2]);
}

struct BinUnit {
  int64_t chunk;
  int first, n, bin;
  int64_t d;
  bool dv;
};

// which (chunk, window) this wave owns; false: a window beyond the last one
__device__ __forceinline__ bool bin_unit(const int4* __restrict__ chunks, int64_t D, int Dw, BinUnit& u) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = (int)(threadIdx.x & 63);
  const int Dw4 = (Dw + 3) >> 2;
  u.chunk = (int64_t)blockIdx.x / Dw4;
  const int w = (int)(blockIdx.x % Dw4) * 4 + wave;
  if (w >= Dw) return false;
  const int4 c = chunks[u.chunk];
  u.bin = c.x;
  u.first = c.y;
  u.n = c.z;
  u.d = (int64_t)w * 64 + lane;
  u.dv = u.d < D;
  return true;
}

// ---- 1. moments sweep: cm[chunk][NF][J][Dpad] = sum over the chunk's rows of T_j(s_row) x[row][d] -------------------
// field `sfield` is scaled per column on load (theta = T colscale, as project_kernel does)
template <typename T, int NF, int J>
__global__ void __launch_bounds__(256)
bin_moments_kernel(FieldPtrs<NF> fp, int64_t D, int Dw, const int4* __restrict__ chunks, const int* __restrict__ rows,
                   const double* __restrict__ ss, const double* __restrict__ colscale, int sfield,
                   double* __restrict__ cm) {
  BinUnit u;
  if (!bin_unit(chunks, D, Dw, u)) return;
  const int64_t Dpad = (int64_t)Dw * 64;
  const T* fb[NF];
  double sc[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    fb[f] = reinterpret_cast<const T*>(fp.p[f]) + u.d;
    sc[f] = (colscale != nullptr && f == sfield && u.dv) ? colscale[u.d] : 1.0;
  }
  double m[NF][J];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int j = 0; j < J; ++j) m[f][j] = 0.0;

  auto rows_step = [&](int i, auto nrows_c) {
    constexpr int NR = decltype(nrows_c)::value;
    double x[NR][NF], s[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t ro = (int64_t)rows[u.first + i + r] * D;
      s[r] = ss[u.first + i + r];
#pragma unroll
      for (int f = 0; f < NF; ++f) x[r][f] = u.dv ? (double)fb[f][ro] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      double t[J];
      bin_cheb<J>(s[r], t);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const double xv = x[r][f] * sc[f];
#pragma unroll
        for (int j = 0; j < J; ++j) m[f][j] = fma(t[j], xv, m[f][j]);
      }
    }
  };
  int i = 0;
  for (; i + BIN_UNROLL <= u.n; i += BIN_UNROLL) rows_step(i, std::integral_constant<int, BIN_UNROLL>{});
  for (; i < u.n; ++i) rows_step(i, std::integral_constant<int, 1>{});

  double* o = cm + (u.chunk * NF * J) * Dpad + u.d;      // lanes beyond D store their zeros inside the padding
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int j = 0; j < J; ++j) o[(int64_t)(f * J + j) * Dpad] = m[f][j];
}

// ---- 4. eddy-moments sweep: xbar = sum_j T_j(s_row) z[bin][f][j], eddies x - xbar, the products u'v', u'omega',
// v'theta' (tem_diagnostics.py:517-529, 547-555) and their J moments per chunk: cm[chunk][3][J][Dpad] ---------------
template <typename T, int J>
__global__ void __launch_bounds__(256, 2)
bin_eddy_moments_kernel(FieldPtrs<4> fp, int64_t D, int Dw, const int4* __restrict__ chunks, const int* __restrict__ rows,
                        const double* __restrict__ ss, const double* __restrict__ colscale, const double* __restrict__ z,
                        double* __restrict__ cm) {
  BinUnit u;
  if (!bin_unit(chunks, D, Dw, u)) return;
  const int64_t Dpad = (int64_t)Dw * 64;
  const T* fb[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) fb[f] = reinterpret_cast<const T*>(fp.p[f]) + u.d;
  const double sth = (colscale != nullptr && u.dv) ? colscale[u.d] : 1.0;
  double zr[4][J], m[3][J];
  const double* zb = z + ((int64_t)u.bin * 4 * J) * Dpad + u.d;
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int j = 0; j < J; ++j) zr[f][j] = u.dv ? zb[(int64_t)(f * J + j) * Dpad] : 0.0;
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int j = 0; j < J; ++j) m[q][j] = 0.0;

  auto rows_step = [&](int i, auto nrows_c) {
    constexpr int NR = decltype(nrows_c)::value;
    double x[NR][4], s[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int64_t ro = (int64_t)rows[u.first + i + r] * D;
      s[r] = ss[u.first + i + r];
#pragma unroll
      for (int f = 0; f < 4; ++f) x[r][f] = u.dv ? (double)fb[f][ro] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      double t[J], e[4];
      bin_cheb<J>(s[r], t);
      x[r][2] *= sth;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        double xb = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) xb = fma(t[j], zr[f][j], xb);
        e[f] = x[r][f] - xb;
      }
      const double p[3] = {e[0] * e[1], e[0] * e[3], e[1] * e[2]};
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int j = 0; j < J; ++j) m[q][j] = fma(t[j], p[q], m[q][j]);
    }
  };
  int i = 0;
  for (; i + BIN_UNROLL <= u.n; i += BIN_UNROLL) rows_step(i, std::integral_constant<int, BIN_UNROLL>{});
  for (; i < u.n; ++i) rows_step(i, std::integral_constant<int, 1>{});

  double* o = cm + (u.chunk * 3 * J) * Dpad + u.d;
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int j = 0; j < J; ++j) o[(int64_t)(q * J + j) * Dpad] = m[q][j];
}

// bins [b0, b1) of slab `sl` of `nsl`
__device__ __forceinline__ void bin_slab(int B, int nsl, int sl, int& b0, int& b1) {
  b0 = (int)((int64_t)B * sl / nsl);
  b1 = (int)((int64_t)B * (sl + 1) / nsl);
}

// ---- 2. chunk -> bin reduction and the per-bin contraction --------------------------------------------------------
// partial[slab][f][k][d] = sum over the slab's bins, j:  a[bin][j][k] (sum over the bin's chunks of cm[chunk][f][j][d])
// grid (Dw, NF, slabs), one wave per workgroup, one column d per lane, K accumulators per lane
template <int KP>
__global__ void __launch_bounds__(64)
bin_contract_kernel(const double* __restrict__ cm, int NF, int J, int64_t D, int Dw, int B, int K,
                    const int* __restrict__ bin_chunk0, const double* __restrict__ a, double* __restrict__ partial) {
  const int64_t Dpad = (int64_t)Dw * 64;
  const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int f = blockIdx.y, sl = blockIdx.z;
  int b0, b1;
  bin_slab(B, gridDim.z, sl, b0, b1);
  double acc[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) acc[k] = 0.0;
  for (int b = b0; b < b1; ++b) {
    const int c0 = bin_chunk0[b], c1 = bin_chunk0[b + 1];
    if (c0 == c1) continue;
    for (int j = 0; j < J; ++j) {
      double mm = 0.0;
      for (int c = c0; c < c1; ++c) mm += cm[(((int64_t)c * NF + f) * J + j) * Dpad + d];
      const double* ar = a + ((int64_t)b * J + j) * KP;
#pragma unroll
      for (int k = 0; k < KP; ++k) acc[k] = fma(ar[k], mm, acc[k]);
    }
  }
  if (d < D) {
    double* o = partial + (((int64_t)sl * NF + f) * K) * D + d;
#pragma unroll
    for (int k = 0; k < KP; ++k)
      if (k < K) o[(int64_t)k * D] = acc[k];
  }
}

// ---- change of basis of K coefficients per column, in place or not: out[f][o][d] = sum_i M[o][i] in[f][i][d] --------
// M is [KP][KP], zero padded (T^T: sums in the Y basis -> the plan's Q basis; T: coefficients in Q -> in Y).
// grid (ceil(D / 64), NF); a lane reads its whole column before it writes
template <int KP>
__global__ void __launch_bounds__(64)
bin_basis_kernel(const double* in, int64_t in_rows, const double* __restrict__ M, int K, int64_t D, double* out,
                 int64_t out_rows) {
  const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (d >= D) return;
  const double* x = in + (int64_t)blockIdx.y * in_rows * D + d;
  double* y = out + (int64_t)blockIdx.y * out_rows * D + d;
  double v[KP];
#pragma unroll
  for (int i = 0; i < KP; ++i) v[i] = i < K ? x[(int64_t)i * D] : 0.0;
  for (int o = 0; o < K; ++o) {
    const double* mr = M + (int64_t)o * KP;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < KP; ++i) s = fma(mr[i], v[i], s);
    y[(int64_t)o * D] = s;
  }
}

// ---- 3. per-bin synthesis: z[bin][f][j][d] = sum_k a[bin][j][k] cY[f][k][d] for the bins that hold rows ------------
// grid (Dw, NF, slabs); the padding lanes of z are written as zeros
template <int KP>
__global__ void __launch_bounds__(64)
bin_synth_kernel(const double* __restrict__ cY, int NF, int J, int64_t D, int Dw, int B, int K,
                 const int* __restrict__ bin_chunk0, const double* __restrict__ a, double* __restrict__ z) {
  const int64_t Dpad = (int64_t)Dw * 64;
  const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int f = blockIdx.y;
  int b0, b1;
  bin_slab(B, gridDim.z, blockIdx.z, b0, b1);
  double c[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) c[k] = (k < K && d < D) ? cY[((int64_t)f * K + k) * D + d] : 0.0;
  for (int b = b0; b < b1; ++b) {
    if (bin_chunk0[b] == bin_chunk0[b + 1]) continue;
    for (int j = 0; j < J; ++j) {
      const double* ar = a + ((int64_t)b * J + j) * KP;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < KP; ++k) s = fma(ar[k], c[k], s);
      z[(((int64_t)b * NF + f) * J + j) * Dpad + d] = s;
    }
  }
}

// ---- 5. native zonal mean of the operator: out[row][d] = sum_j T_j(s_row) z[bin][j][d] (NF = 1) ----------------------
template <int J>
__global__ void __launch_bounds__(256)
bin_native_kernel(int64_t D, int Dw, const int4* __restrict__ chunks, const int* __restrict__ rows,
                  const double* __restrict__ ss, const double* __restrict__ z, double* __restrict__ out) {
  BinUnit u;
  if (!bin_unit(chunks, D, Dw, u)) return;
  if (!u.dv) return;
  const int64_t Dpad = (int64_t)Dw * 64;
  double zr[J];
  const double* zb = z + ((int64_t)u.bin * J) * Dpad + u.d;
#pragma unroll
  for (int j = 0; j < J; ++j) zr[j] = zb[(int64_t)j * Dpad];
  for (int i = 0; i < u.n; ++i) {
    double t[J];
    bin_cheb<J>(ss[u.first + i], t);
    double xb = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) xb = fma(t[j], zr[j], xb);
    out[(int64_t)rows[u.first + i] * D + u.d] = xb;
  }
}

}  // namespace temx

#endif
