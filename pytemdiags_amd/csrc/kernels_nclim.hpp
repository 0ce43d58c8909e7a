// kernels_nclim.hpp -- the sum over the valid times of fields with missing values (include/temx_nclim.h,
// temxn_time_sum_valid).
//
// NF sources [ncol][nlev][nt] (time fastest, one dtype for the call) -> NF fp64 sums and the counts of the valid
// times, [ncol][nlev] each.  An element is valid iff it is finite; under a common mask a time of a row is valid iff it
// is valid in every field.  Every source element is read from HBM once, in both modes; fp32 widens exactly, every
// addition is fp64, and a value that is not valid is never added.
//
// The kernels are those of kernels_clim.hpp with NFT fields per workgroup (nclim_shapes.hpp cuts the launch from nt,
// the element size and the fields a workgroup holds):
//   NFT = 1        own-mask mode: a field per workgroup, the fields along blockIdx.y.  What a row's sum is does not
//                  depend on what else the call carries.
//   NFT = 4 or 8   common-mask mode, nf <= NFT: the workgroup holds its rows of all nf fields (staged: one LDS image
//                  per field, `img` elements apart; long rows: the nf values of a time in registers) before it adds.
//   staged    load side as time_sum_staged_body, once per field: the lanes run along the span across row boundaries,
//             element loads up to the first 16-byte boundary, 16-byte loads over the body, element loads at the ragged
//             end, CLIM_BATCH vectors in flight per lane.  sum side: g lanes per row; lane j visits the times j, j + g,
//             j + 2g ... in that order, reads the nf values of a time, and where all are finite adds each to its
//             field's accumulator and one to the count; then a butterfly over the g lanes.
//   long row  a wave per row: lane l visits the times l + 64 (4 i + q), accumulator q per field, i ascending;
//             (a0 + a1) + (a2 + a3); the butterfly over 64 lanes.
// Accumulators start from -0.0, the identity of IEEE addition, so a row of one valid element comes out bit for bit, and
// a row with none gives -0.0 and count 0.  Counts are added as integers (nt <= 2^31) and stored as doubles.  Under
// `accumulate` the stored values are acc + sum and cnt + count.  Each row is stored once, by one lane; nothing else
// is written.  All global offsets are int64_t.
#pragma once
#include "kernels_clim.hpp"
#include "nclim_shapes.hpp"
#include <hip/hip_runtime.h>

#include <cstdint>

namespace temx {

struct NclimPtrs {
  const void* src[NCLIM_NFMAX];
  double* acc[NCLIM_NFMAX];
  double* cnt[NCLIM_NFMAX];   // common-mask mode: cnt[0] only
};

__device__ __forceinline__ bool nclim_valid(double x) {
  return (__double_as_longlong(x) & 0x7ff0000000000000ll) != 0x7ff0000000000000ll;
}
__device__ __forceinline__ bool nclim_valid(float x) { return (__float_as_int(x) & 0x7f800000) != 0x7f800000; }

__device__ __forceinline__ int nclim_butterfly(int c, int g) {
  for (int o = g >> 1; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// the pointers of a workgroup: field blockIdx.y alone (NFT = 1) or the first NFT fields
template <int NFT>
__device__ __forceinline__ void nclim_select(const NclimPtrs& fp, const void* (&src)[NFT], double* (&acc)[NFT], double*& cnt) {
  if (NFT == 1) {
    const int f = blockIdx.y;
    src[0] = nullptr, acc[0] = nullptr, cnt = nullptr;
#pragma unroll
    for (int q = 0; q < NCLIM_NFMAX; ++q)
      if (q == f) src[0] = fp.src[q], acc[0] = fp.acc[q], cnt = fp.cnt[q];
  } else {
#pragma unroll
    for (int q = 0; q < NFT; ++q) src[q] = fp.src[q], acc[q] = fp.acc[q];
    cnt = fp.cnt[0];
  }
}

// load side of one field: span element e of p -> s[(e / nt) * stride + e % nt]   (time_sum_staged_body's, n elements)
template <typename T>
__device__ __forceinline__ void nclim_stage(const T* __restrict__ p, T* __restrict__ s, int n, int nt, int stride, int tid) {
  using V = typename ClimVec<T>::type;
  constexpr int VN = ClimVec<T>::N;
  int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(T));   // elements before the first 16-byte boundary
  if (head > n) head = n;
  const int nvec = (n - head) / VN;
  const int tail0 = head + nvec * VN;
  const V* pv = reinterpret_cast<const V*>(p + head);
  for (int vb = tid; vb < nvec; vb += NCLIM_THREADS * CLIM_BATCH) {
    V v[CLIM_BATCH];
#pragma unroll
    for (int q = 0; q < CLIM_BATCH; ++q) {
      const int i = vb + q * NCLIM_THREADS;
      if (i < nvec) v[q] = pv[i];
    }
#pragma unroll
    for (int q = 0; q < CLIM_BATCH; ++q) {
      const int i = vb + q * NCLIM_THREADS;
      if (i < nvec) {
        const int e = head + i * VN;
        int r = e / nt, t = e - r * nt;
#pragma unroll
        for (int k = 0; k < VN; ++k) {
          s[r * stride + t] = ClimVec<T>::get(v[q], k);
          if (++t == nt) t = 0, ++r;
        }
      }
    }
  }
  for (int e = tid; e < head; e += NCLIM_THREADS) {        // head: fewer than 16 / sizeof(T) elements
    const int r = e / nt;
    s[r * stride + (e - r * nt)] = p[e];
  }
  for (int e = tail0 + tid; e < n; e += NCLIM_THREADS) {   // ragged end: fewer than 16 / sizeof(T) elements
    const int r = e / nt;
    s[r * stride + (e - r * nt)] = p[e];
  }
}

// grid (ceil(rows / sh.rpb), NFT == 1 ? nf : 1)
template <typename T, int NFT>
__global__ void __launch_bounds__(NCLIM_THREADS)
time_sum_valid_staged_kernel(NclimPtrs fp, int nf, int64_t rows, int nt, NclimShape sh, int accumulate) {
  __shared__ __attribute__((aligned(16))) unsigned char nclim_lds[NCLIM_LDS_BYTES];
  const void* srcv[NFT];
  double* acc[NFT];
  double* cnt;
  nclim_select<NFT>(fp, srcv, acc, cnt);
  const int nfs = NFT == 1 ? 1 : nf;                       // fields of this workgroup
  const int rpb = sh.rpb, stride = sh.stride, g = sh.g;
  const int img = rpb * stride;                            // elements of one field's image: nfs * img * sizeof(T) <= NCLIM_LDS_BYTES
  T* s = reinterpret_cast<T*>(nclim_lds);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  if (r0 >= rows) return;   // (uniform; the host launches exactly ceil(rows / rpb) workgroups along x)
  const int nr = (int)(rows - r0 < rpb ? rows - r0 : rpb);        // valid rows of this workgroup
  const int tid = threadIdx.x;
#pragma unroll
  for (int f = 0; f < NFT; ++f)
    if (f < nfs) nclim_stage<T>(reinterpret_cast<const T*>(srcv[f]) + r0 * nt, s + f * img, nr * nt, nt, stride, tid);
  __syncthreads();

  // ---- sum side: g lanes per row, rpb * g <= NCLIM_THREADS, a row's lanes inside one wave ----
  const int r = tid / g, j = tid - r * g;
  double a[NFT];
#pragma unroll
  for (int f = 0; f < NFT; ++f) a[f] = -0.0;
  int c = 0;
  if (r < nr) {
    const T* sr = s + r * stride;
    for (int t = j; t < nt; t += g) {
      T x[NFT];
      bool ok = true;
#pragma unroll
      for (int f = 0; f < NFT; ++f)
        if (f < nfs) x[f] = sr[f * img + t], ok = ok && nclim_valid(x[f]);
      if (ok) {
#pragma unroll
        for (int f = 0; f < NFT; ++f)
          if (f < nfs) a[f] += (double)x[f];
        ++c;
      }
    }
  }
#pragma unroll
  for (int f = 0; f < NFT; ++f)
    if (f < nfs) a[f] = clim_butterfly(a[f], g);
  c = nclim_butterfly(c, g);
  if (r < nr && j == 0) {
    const int64_t row = r0 + r;
#pragma unroll
    for (int f = 0; f < NFT; ++f)
      if (f < nfs) acc[f][row] = accumulate ? acc[f][row] + a[f] : a[f];
    cnt[row] = accumulate ? cnt[row] + (double)c : (double)c;
  }
}

// grid (ceil(rows / NCLIM_LONG_ROWS), NFT == 1 ? nf : 1): a wave per row
template <typename T, int NFT>
__global__ void __launch_bounds__(NCLIM_THREADS)
time_sum_valid_long_kernel(NclimPtrs fp, int nf, int64_t rows, int64_t nt, int accumulate) {
  const void* srcv[NFT];
  double* acc[NFT];
  double* cnt;
  nclim_select<NFT>(fp, srcv, acc, cnt);
  const int nfs = NFT == 1 ? 1 : nf;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * NCLIM_LONG_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;   // (uniform per wave)
  const T* p[NFT];
#pragma unroll
  for (int f = 0; f < NFT; ++f) p[f] = reinterpret_cast<const T*>(srcv[f]) + row * nt;
  double a[NFT][4];
#pragma unroll
  for (int f = 0; f < NFT; ++f)
#pragma unroll
    for (int q = 0; q < 4; ++q) a[f][q] = -0.0;
  int c = 0;
  for (int64_t t = lane; t < nt; t += 256) {
    // (loads first: four times of every field in flight per lane; a field beyond nfs reads nothing and counts as valid)
    T x[4][NFT];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool k = t + 64 * q < nt;
#pragma unroll
      for (int f = 0; f < NFT; ++f) x[q][f] = (k && f < nfs) ? p[f][t + 64 * q] : (T)0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bool ok = t + 64 * q < nt;
#pragma unroll
      for (int f = 0; f < NFT; ++f) ok = ok && nclim_valid(x[q][f]);
      if (ok) {
#pragma unroll
        for (int f = 0; f < NFT; ++f) a[f][q] += (double)x[q][f];
        ++c;
      }
    }
  }
  c = nclim_butterfly(c, 64);
#pragma unroll
  for (int f = 0; f < NFT; ++f)
    if (f < nfs) {
      const double v = clim_butterfly((a[f][0] + a[f][1]) + (a[f][2] + a[f][3]), 64);
      if (lane == 0) acc[f][row] = accumulate ? acc[f][row] + v : v;
    }
  if (lane == 0) cnt[row] = accumulate ? cnt[row] + (double)c : (double)c;
}

}  // namespace temx
