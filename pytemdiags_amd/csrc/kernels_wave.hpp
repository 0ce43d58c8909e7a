// kernels_wave.hpp -- gfx950 device code of the zonal-wavenumber fit (pytemdiags_amd/include/temx_wave.h; the host side
// of the tables is wave_tables.hpp).  Vocabulary of kernels.hpp, plus: m a zonal wavenumber, ndeg = L + 1 - m degrees,
// Kc = 2 ndeg basis columns (cos half, then sin half), Ym [N][Kc] the basis at the native columns, Pz [M][ndeg] the
// Pbar_l^m at the output latitudes.
//
// The projection itself is project_kernel of kernels.hpp (one wave per d-tile and field, basis blocks staged through LDS,
// fields loaded straight into the MFMA B layout, splits over chunk ranges, the deterministic slab reduction): it is
// handed the blocked basis written here instead of the plan's.  What it streams is not Ym but the DEFLATED basis
//     Ymd = (I - P) Ym,      P = Y0 pinv(Y0) the plan's native zonal-mean operator (symmetric),
// so that Ymd^T x = Ym^T (x - P x) = Ym^T x': the fit of the eddy costs one sweep over the raw fields per wavenumber and
// neither the eddy nor the zonal-mean coefficients of the fields are ever formed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace temx {

// Pbar_l^m(x), l = m .. L, by the normalised three-term recurrence (wave_pbar_row of wave_tables.hpp); f(l - m, value)
// is called in ascending l.  pmm_norm = (-1)^m sqrt(2) sqrt((2m+1)/(4 pi) prod (2k-1)/(2k)) comes from the host.
// cos(lat) is taken from x, sqrt(1 - x^2): the row is a function of x alone, as on the host and in scipy's lpmv.
template <typename F>
__device__ __forceinline__ void wave_pbar_each(int m, int L, double x, double pmm_norm, F&& f) {
  double cm = 1.0, cb = sqrt(1.0 - x * x);
  for (int e = m; e > 0; e >>= 1) {       // c^m by squaring
    if (e & 1) cm *= cb;
    cb *= cb;
  }
  const double pmm = pmm_norm * cm;
  f(0, pmm);
  if (L == m) return;
  double p2 = pmm, p1 = sqrt(2.0 * m + 3.0) * x * pmm;
  f(1, p1);
  const double m2 = (double)m * m;
  for (int l = m + 2; l <= L; ++l) {
    const double l2 = (double)l * l, q = (double)(l - 1) * (l - 1);
    const double a = sqrt((4.0 * l2 - 1.0) / (l2 - m2));
    const double b = sqrt((q - m2) / (4.0 * q - 1.0));
    const double p = a * (x * p1 - b * p2);
    p2 = p1;
    p1 = p;
    f(l - m, p);
  }
}

// One thread per native column (rows N .. nrow_pad are padding).  Writes the row-major Ym [N][Kc] (the "field" of the
// build-time Gram sweep and of the deflation) and the 4x4-blocked copy the sweep streams as MFMA A operands,
//   yblk[group][t][k*4 + i] = Ym[4 group + k][4 t + i]        (t < gstride, 128 B per block),
// with rows >= N and columns >= Kc zero, as basis_kernel does.
__global__ void __launch_bounds__(256)
wave_basis_kernel(const double* __restrict__ lat_rad, const double* __restrict__ lon_rad, int64_t N, int64_t nrow_pad,
                  int m, int L, double pmm_norm, int gstride, double* __restrict__ Ym, double* __restrict__ yblk) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nrow_pad) return;
  const int ndeg = L + 1 - m, Kc = 2 * ndeg;
  double* blk = yblk + (i >> 2) * (int64_t)gstride * 16 + (int)(i & 3) * 4;
  auto put = [&](int col, double v) { blk[(col >> 2) * 16 + (col & 3)] = v; };
  if (i >= N) {
    for (int col = 0; col < 4 * gstride; ++col) put(col, 0.0);
    return;
  }
  const double phi = lat_rad[i], lam = lon_rad[i];
  const double cs = cos(m * lam), sn = sin(m * lam);
  double* row = Ym + i * Kc;
  wave_pbar_each(m, L, sin(phi), pmm_norm, [&](int j, double p) {
    const double vc = p * cs, vs = p * sn;
    row[j] = vc;
    row[ndeg + j] = vs;
    put(j, vc);
    put(ndeg + j, vs);
  });
  for (int col = Kc; col < 4 * gstride; ++col) put(col, 0.0);
}

// Pz[j][l - m] = Pbar_l^m(sin lat_out_j): one thread per output latitude
__global__ void __launch_bounds__(256)
wave_ztable_kernel(const double* __restrict__ lat_out_rad, int M, int m, int L, double pmm_norm, double* __restrict__ Pz) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  const int ndeg = L + 1 - m;
  const double phi = lat_out_rad[j];
  double* row = Pz + (int64_t)j * ndeg;
  wave_pbar_each(m, L, sin(phi), pmm_norm, [&](int k, double p) { row[k] = p; });
}

// the blocked copy becomes the deflated basis: yblk(i, k) = Ym[i][k] - Z[i][k], Z = P Ym [N][Kc]
__global__ void __launch_bounds__(256)
wave_deflate_kernel(const double* __restrict__ Ym, const double* __restrict__ Z, int64_t N, int Kc, int gstride,
                    double* __restrict__ yblk) {
  const int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (idx >= N * Kc) return;
  const int64_t i = idx / Kc;
  const int k = (int)(idx - i * Kc);
  yblk[((i >> 2) * gstride + (k >> 2)) * 16 + (int)(i & 3) * 4 + (k & 3)] = Ym[idx] - Z[idx];
}

// C[f][k][d] = sum_j Ginv[k][j] B[f][j][d]: the normal equations of the fit, Gm c = Ym^T x'.  One thread per (k, d),
// a block is 4 rows x 64 columns: the loads of B are coalesced along d, a row of Ginv is a broadcast.
__global__ void __launch_bounds__(256)
wave_solve_kernel(const double* __restrict__ B, int Kc, int64_t D, const double* __restrict__ Ginv, double* __restrict__ C) {
  const int64_t d = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int k = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int f = blockIdx.z;
  if (d >= D || k >= Kc) return;
  const double* b = B + (int64_t)f * Kc * D + d;
  const double* g = Ginv + (int64_t)k * Kc;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;      // four chains: the dot is latency bound
  int j = 0;
  for (; j + 4 <= Kc; j += 4) {
    v0 += g[j] * b[(int64_t)j * D];
    v1 += g[j + 1] * b[(int64_t)(j + 1) * D];
    v2 += g[j + 2] * b[(int64_t)(j + 2) * D];
    v3 += g[j + 3] * b[(int64_t)(j + 3) * D];
  }
  for (; j < Kc; ++j) v0 += g[j] * b[(int64_t)j * D];
  C[((int64_t)f * Kc + k) * D + d] = (v0 + v1) + (v2 + v3);
}

// cos and sin part of one field's wave-m component at output latitude j, column d:
//   Xc = sum_l a_l Pz[j][l],  Xs = sum_l b_l Pz[j][l],   a = C[0 .. ndeg), b = C[ndeg .. Kc), l ascending
__device__ __forceinline__ void wave_parts_at(const double* __restrict__ C, const double* __restrict__ pz, int ndeg,
                                              int64_t D, double& xc, double& xs) {
  double a = 0.0, b = 0.0;
  for (int l = 0; l < ndeg; ++l) {
    const double p = pz[l];
    a += C[(int64_t)l * D] * p;
    b += C[(int64_t)(ndeg + l) * D] * p;
  }
  xc = a;
  xs = b;
}

// parts[f][2][M][D] of nf fields (the operator alone): one thread per (j, d), blockIdx.z = field
__global__ void __launch_bounds__(256)
wave_parts_kernel(const double* __restrict__ C, int ndeg, int M, int64_t D, const double* __restrict__ Pz,
                  double* __restrict__ parts) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y, f = blockIdx.z;
  if (d >= D) return;
  double xc, xs;
  wave_parts_at(C + (int64_t)f * 2 * ndeg * D + d, Pz + (int64_t)j * ndeg, ndeg, D, xc, xs);
  const int64_t MD = (int64_t)M * D;
  parts[(int64_t)f * 2 * MD + (int64_t)j * D + d] = xc;
  parts[((int64_t)f * 2 + 1) * MD + (int64_t)j * D + d] = xs;
}

// The three wave-m fluxes on the zonal grid, [x'_m y'_m] = (Xc Yc + Xs Ys) / 2 for (u, v), (u, omega), (v, theta), from
// the coefficient slab C[4][Kc][D] (u, v, theta, omega) and Pz; on request the eight parts [4][2][M][D].  One thread per
// (j, d); the fluxes are the same bits with and without the parts.
__global__ void __launch_bounds__(256)
wave_flux_kernel(const double* __restrict__ C, int ndeg, int M, int64_t D, const double* __restrict__ Pz,
                 double* __restrict__ flux, double* __restrict__ parts) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.y;
  if (d >= D) return;
  const int64_t MD = (int64_t)M * D, o = (int64_t)j * D + d;
  double xc[4], xs[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    wave_parts_at(C + (int64_t)f * 2 * ndeg * D + d, Pz + (int64_t)j * ndeg, ndeg, D, xc[f], xs[f]);
    if (parts != nullptr) {
      parts[(int64_t)f * 2 * MD + o] = xc[f];
      parts[((int64_t)f * 2 + 1) * MD + o] = xs[f];
    }
  }
  flux[o] = 0.5 * (xc[0] * xc[1] + xs[0] * xs[1]);            // u'v'
  flux[MD + o] = 0.5 * (xc[0] * xc[3] + xs[0] * xs[3]);       // u'omega'
  flux[2 * MD + o] = 0.5 * (xc[1] * xc[2] + xs[1] * xs[2]);   // v'theta'
}

}  // namespace temx
