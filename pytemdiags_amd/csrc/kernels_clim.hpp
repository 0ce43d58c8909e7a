// kernels_clim.hpp -- the sum over time of fields in the engine's layout (include/temx_clim.h, temxc_time_sum).
//
// NF sources [ncol][nlev][nt] (time fastest, fp64 or fp32 each) -> NF fp64 accumulators [ncol][nlev].  A field is
// R = ncol * nlev rows of nt elements back to back, no padding: a row starts on a 16-byte boundary only by luck.
// Every element is read once; fp32 widens exactly and every addition is fp64.
//
// The sum of a row is a fixed function of its nt values, nt and dtype (clim_shapes.hpp picks the kernel and its shape
// from nt and the element size alone; the fp64 and the fp32 sources of a call go in a launch each):
//   staged    (time_sum_staged_kernel) a workgroup owns rpb consecutive rows, one contiguous span of the source.
//             load side: the lanes run along the span across row boundaries: element loads up to the first 16-byte
//             boundary, 16-byte loads over the body, element loads at the ragged end, CLIM_BATCH vectors in flight per
//             lane before the first goes to LDS.  The LDS image keeps the source dtype, a row every `stride` elements,
//             stride odd: the lanes that then read one time of neighbouring rows fall into different banks.
//             sum side: g lanes per row (a power of two, inside one wave); lane j adds the times j, j + g, j + 2g ... in
//             that order, then a butterfly over the g lanes (IEEE addition commutes, so every lane of the butterfly
//             holds the same bits).
//   long row  (time_sum_long_kernel) a wave per row: lane l adds the times l + 64 (4 i + q) into accumulator q, i
//             ascending; (a0 + a1) + (a2 + a3); the same butterfly over 64 lanes.  Loads are element loads, a wave
//             instruction covers 64 consecutive elements.
// Accumulators start from -0.0, the identity of IEEE addition (x + -0.0 == x for every x, -0.0 included), so a row
// of one element comes out bit for bit.  Under `accumulate` the stored value is acc + sum, one further rounding.
// Nothing is written outside acc[f][0 .. R): each row is stored once, by one lane.  All global offsets are int64_t.
#pragma once
#include "clim_shapes.hpp"
#include <hip/hip_runtime.h>

#include <cstdint>

namespace temx {

constexpr int CLIM_BATCH = 4;   // 16-byte loads in flight per lane on the load side

struct ClimPtrs {
  const void* src[CLIM_NFMAX];
  double* acc[CLIM_NFMAX];
};

__device__ __forceinline__ double clim_butterfly(double a, int g) {
  for (int o = g >> 1; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  return a;
}

template <typename T>
struct ClimVec;
template <>
struct ClimVec<double> {
  using type = double2;
  static constexpr int N = 2;
  static __device__ __forceinline__ double get(const double2& v, int q) { return q ? v.y : v.x; }
};
template <>
struct ClimVec<float> {
  using type = float4;
  static constexpr int N = 4;
  static __device__ __forceinline__ float get(const float4& v, int q) { return q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w; }
};

// the sum side of the plain time sum: the one written out in time_sum_staged_body
struct ClimPlainSum {
  static constexpr bool plain = true;
};

// one workgroup of the staged kernel, for a source of element type T.  lds: CLIM_LDS_BYTES, 16-byte aligned.
// SUM: ClimPlainSum, or the sum side of another kernel that shares this load side (kernels_gclim.hpp): an object whose
// sum(s, nr, r0, stride, acc, accumulate, tid) runs once the rows lie in LDS.
template <typename T, typename SUM = ClimPlainSum>
__device__ __forceinline__ void time_sum_staged_body(const T* __restrict__ src, double* __restrict__ acc, int64_t rows,
                                                     int nt, int rpb, int stride, int g, int accumulate,
                                                     unsigned char* lds, const SUM& other = SUM{}) {
  using V = typename ClimVec<T>::type;
  constexpr int VN = ClimVec<T>::N;
  T* s = reinterpret_cast<T*>(lds);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  if (r0 >= rows) return;   // (uniform; the host launches exactly ceil(rows / rpb) workgroups per field)
  const int nr = (int)(rows - r0 < rpb ? rows - r0 : rpb);       // valid rows of this workgroup
  const int n = nr * nt;                                         // elements of its span (<= CLIM_LDS_BYTES / sizeof(T))
  const T* p = src + r0 * nt;
  const int tid = threadIdx.x;

  // ---- load side: span element e -> s[(e / nt) * stride + e % nt] ----
  int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(T));   // elements before the first 16-byte boundary
  if (head > n) head = n;
  const int nvec = (n - head) / VN;
  const int tail0 = head + nvec * VN;
  const V* pv = reinterpret_cast<const V*>(p + head);
  for (int vb = tid; vb < nvec; vb += CLIM_THREADS * CLIM_BATCH) {
    V v[CLIM_BATCH];
#pragma unroll
    for (int q = 0; q < CLIM_BATCH; ++q) {
      const int i = vb + q * CLIM_THREADS;
      if (i < nvec) v[q] = pv[i];
    }
#pragma unroll
    for (int q = 0; q < CLIM_BATCH; ++q) {
      const int i = vb + q * CLIM_THREADS;
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
  for (int e = tid; e < head; e += CLIM_THREADS) {     // head: fewer than 16 / sizeof(T) elements
    const int r = e / nt;
    s[r * stride + (e - r * nt)] = p[e];
  }
  for (int e = tail0 + tid; e < n; e += CLIM_THREADS) {   // ragged end: fewer than 16 / sizeof(T) elements
    const int r = e / nt;
    s[r * stride + (e - r * nt)] = p[e];
  }
  __syncthreads();

  if constexpr (!SUM::plain) {
    other.sum(s, nr, r0, stride, acc, accumulate, tid);
    return;
  }
  // ---- sum side: g lanes per row, rpb * g <= CLIM_THREADS, a row's lanes inside one wave ----
  const int r = tid / g, j = tid - r * g;
  double a = -0.0;
  if (r < nr) {
    const T* sr = s + r * stride;
    for (int t = j; t < nt; t += g) a += (double)sr[t];
  }
  a = clim_butterfly(a, g);
  if (r < nr && j == 0) {
    double* o = acc + r0 + r;
    *o = accumulate ? *o + a : a;
  }
}

// grid (ceil(rows / sh.rpb), nf): the nf sources of one launch share the element type T
template <typename T>
__global__ void __launch_bounds__(CLIM_THREADS)
time_sum_staged_kernel(ClimPtrs fp, int64_t rows, int nt, ClimShape sh, int accumulate) {
  __shared__ __attribute__((aligned(16))) unsigned char clim_lds[CLIM_LDS_BYTES];
  const int f = blockIdx.y;
  const void* srcv = nullptr;
  double* acc = nullptr;
#pragma unroll
  for (int q = 0; q < CLIM_NFMAX; ++q)
    if (q == f) srcv = fp.src[q], acc = fp.acc[q];
  time_sum_staged_body<T>(reinterpret_cast<const T*>(srcv), acc, rows, nt, sh.rpb, sh.stride, sh.g, accumulate, clim_lds);
}

template <typename T>
__device__ __forceinline__ double time_sum_long_row(const T* __restrict__ p, int64_t nt, int lane) {
  double a0 = -0.0, a1 = -0.0, a2 = -0.0, a3 = -0.0;
  for (int64_t t = lane; t < nt; t += 256) {
    // (loads first: four in flight per lane)
    const bool k1 = t + 64 < nt, k2 = t + 128 < nt, k3 = t + 192 < nt;
    const T x0 = p[t];
    const T x1 = k1 ? p[t + 64] : (T)0;
    const T x2 = k2 ? p[t + 128] : (T)0;
    const T x3 = k3 ? p[t + 192] : (T)0;
    a0 += (double)x0;
    if (k1) a1 += (double)x1;
    if (k2) a2 += (double)x2;
    if (k3) a3 += (double)x3;
  }
  return clim_butterfly((a0 + a1) + (a2 + a3), 64);
}

// grid (ceil(rows / CLIM_LONG_ROWS), nf): a wave per row
template <typename T>
__global__ void __launch_bounds__(CLIM_THREADS)
time_sum_long_kernel(ClimPtrs fp, int64_t rows, int64_t nt, int accumulate) {
  const int f = blockIdx.y;
  const void* srcv = nullptr;
  double* acc = nullptr;
#pragma unroll
  for (int q = 0; q < CLIM_NFMAX; ++q)
    if (q == f) srcv = fp.src[q], acc = fp.acc[q];
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * CLIM_LONG_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;   // (uniform per wave)
  const double a = time_sum_long_row(reinterpret_cast<const T*>(srcv) + row * nt, nt, lane);
  if (lane == 0) acc[row] = accumulate ? acc[row] + a : a;
}

}  // namespace temx
