// kernels_gclim.hpp -- the grouped, weighted sum over time of fields in the engine's layout (include/temx_gclim.h,
// temxg_time_sum_groups).
//
// NF sources [ncol][nlev][nt] (one block of a record, time fastest, fp64 or fp32 each) -> NF fp64 accumulators
// [ncol][nlev][ng].  Every time of the record has a label (-1: left out) and a weight; the block holds the times
// t0 .. t0 + nt.  Every element is read from HBM once; fp32 widens exactly; every step of a sum is one fp64 fma
// a <- w * x + a, so an array of ones gives the bits of plain additions.
//
// The rows are cut as the plain time sum cuts them (clim_shapes.hpp, a function of nt and the element size), and a
// (row, group) sum is a fixed function of the block's values, labels and weights, nt and the dtype:
//   staged    (time_sum_groups_staged_kernel) the load side is that of the plain time sum (time_sum_staged_body): a
//             workgroup's rows lie in LDS, a row every `stride` elements, stride odd.  Sum side: a work item is (group
//             present, row); a wave takes 64 consecutive rows of one group, so the group's list of times (the range
//             lo .. hi of the record's sorted table, gclim_tables.hpp) is wave-uniform and comes through the scalar
//             loads, and the lanes' LDS reads of one time fall into different banks.  A lane walks its group's times in
//             ascending order and stores its sum.
//   long row  (time_sum_groups_long_kernel<T, NGB>) a wave per row: lane l holds the times l + 64 i, i ascending, and
//             one accumulator per group present (at most NGB); for each it takes label == g ? fma(w, x, a_g) : a_g, so
//             a time of another group, or of none, never enters the arithmetic; one butterfly over 64 lanes per group
//             present.  Loads are element loads, a wave instruction covers 64 consecutive elements; labels and weights
//             are read next to them from the record's table (L2 hits after the first row).  Instantiated for NGB = 1
//             and 4; with more groups present the accumulators live in LDS (time_sum_groups_long_lds_kernel, below),
//             same order, same bits.  The groups present pick the kernel and no bit of a sum.
// Sums start from -0.0, the identity of IEEE addition.  Without `accumulate` the groups absent from the block are stored
// as zero; with it they are neither read nor written.  Each output is stored once, by one lane; nothing is written
// outside acc[f][0 .. R * ng).  All global offsets are int64_t.
#pragma once
#include "gclim_tables.hpp"
#include "kernels_clim.hpp"
#include <hip/hip_runtime.h>

#include <cstdint>

namespace temx {

constexpr int GCLIM_CHUNK = 8;   // accumulators of the long-row kernel that share one "in use" test

struct GclimTab {          // the record's table on the device (GclimRecord::image)
  const double* w;         // [nt_record] weights by time
  const double* sw;        // weights in sorted order
  const int32_t* lab;      // [nt_record] labels by time
  const int32_t* st;       // times by (group, time)
};

// the sum side of the staged kernel, run by time_sum_staged_body once a workgroup's rows lie in LDS
template <typename T>
struct GclimStagedSum {
  static constexpr bool plain = false;
  GclimTab tb;
  const GclimWindow* win;   // (the kernel's own argument)
  int t0;

  __device__ __forceinline__ void sum(const T* s, int nr, int64_t r0, int stride, double* __restrict__ acc, int accumulate,
                                      int tid) const {
    // unit = (group present, 64 consecutive rows), one wave per unit
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int chunks = (nr + 63) >> 6;
    const int units = win->np * chunks;
    const int ng = win->ng;
    for (int unit = wave; unit < units; unit += CLIM_THREADS / 64) {
      const int q = unit / chunks;
      const int r = (unit - q * chunks) * 64 + lane;
      const int lo = win->lo[q], hi = win->hi[q], g = win->pg[q];
      if (r < nr) {
        const T* sr = s + r * stride;
        double a = -0.0;
        for (int j = lo; j < hi; ++j) a = __builtin_fma(tb.sw[j], (double)sr[tb.st[j] - t0], a);
        double* o = acc + (r0 + r) * ng + g;
        *o = accumulate ? *o + a : a;
      }
    }
    // the groups absent from the block: zero, unless the call accumulates
    if (!accumulate && win->np < ng) {
      const int n = nr * ng;
      for (int e = tid; e < n; e += CLIM_THREADS) {
        const int g = e % ng;
        if (!((win->mask >> g) & 1ull)) acc[r0 * ng + e] = 0.0;
      }
    }
  }
};

// grid (ceil(rows / sh.rpb), nf): the nf sources of one launch share the element type T
template <typename T>
__global__ void __launch_bounds__(CLIM_THREADS)
time_sum_groups_staged_kernel(ClimPtrs fp, int64_t rows, int nt, int t0, ClimShape sh, GclimTab tb, GclimWindow win,
                              int accumulate) {
  __shared__ __attribute__((aligned(16))) unsigned char gclim_lds[CLIM_LDS_BYTES];
  const int f = blockIdx.y;
  const void* srcv = nullptr;
  double* acc = nullptr;
#pragma unroll
  for (int q = 0; q < CLIM_NFMAX; ++q)
    if (q == f) srcv = fp.src[q], acc = fp.acc[q];
  time_sum_staged_body<T>(reinterpret_cast<const T*>(srcv), acc, rows, nt, sh.rpb, sh.stride, sh.g, accumulate, gclim_lds,
                          GclimStagedSum<T>{tb, &win, t0});
}

// grid (ceil(rows / CLIM_LONG_ROWS), nf): a wave per row, at most NGB groups present in the block
template <typename T, int NGB>
__global__ void __launch_bounds__(CLIM_THREADS)
time_sum_groups_long_kernel(ClimPtrs fp, int64_t rows, int64_t nt, int64_t t0, GclimTab tb, GclimWindow win, int accumulate) {
  const int f = blockIdx.y;
  const void* srcv = nullptr;
  double* acc = nullptr;
#pragma unroll
  for (int q = 0; q < CLIM_NFMAX; ++q)
    if (q == f) srcv = fp.src[q], acc = fp.acc[q];
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * CLIM_LONG_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;   // (uniform per wave)
  const T* __restrict__ p = reinterpret_cast<const T*>(srcv) + row * nt;
  const int32_t* __restrict__ lab = tb.lab + t0;
  const double* __restrict__ w = tb.w + t0;
  constexpr bool DIRECT = NGB == GCLIM_NGMAX;
  double a[NGB];
#pragma unroll
  for (int q = 0; q < NGB; ++q) a[q] = -0.0;
  for (int64_t t = lane; t < nt; t += 256) {
    // (loads first: four in flight per lane; a time beyond the row carries the label of no group)
    const bool k1 = t + 64 < nt, k2 = t + 128 < nt, k3 = t + 192 < nt;
    const T x0 = p[t];
    const T x1 = k1 ? p[t + 64] : (T)0;
    const T x2 = k2 ? p[t + 128] : (T)0;
    const T x3 = k3 ? p[t + 192] : (T)0;
    const int l0 = lab[t];
    const int l1 = k1 ? lab[t + 64] : -1;
    const int l2 = k2 ? lab[t + 128] : -1;
    const int l3 = k3 ? lab[t + 192] : -1;
    const double w0 = w[t];
    const double w1 = k1 ? w[t + 64] : 0.0;
    const double w2 = k2 ? w[t + 128] : 0.0;
    const double w3 = k3 ? w[t + 192] : 0.0;
    // the widest instantiation keeps accumulator q for group q itself (nothing to look up); the others keep it for the
    // q-th group present.  Accumulators go in chunks of GCLIM_CHUNK; a chunk beyond the groups in use is skipped (uniform).
    const int used = DIRECT ? win.ng : win.np;
#pragma unroll
    for (int c = 0; c < NGB; c += GCLIM_CHUNK) {
      if (c < used) {
#pragma unroll
        for (int q = c; q < c + GCLIM_CHUNK && q < NGB; ++q) {
          const int g = DIRECT ? q : win.pg[q];   // (-2 beyond the groups present: matches no label)
          a[q] = l0 == g ? __builtin_fma(w0, (double)x0, a[q]) : a[q];
          a[q] = l1 == g ? __builtin_fma(w1, (double)x1, a[q]) : a[q];
          a[q] = l2 == g ? __builtin_fma(w2, (double)x2, a[q]) : a[q];
          a[q] = l3 == g ? __builtin_fma(w3, (double)x3, a[q]) : a[q];
        }
      }
    }
  }
  // lane g of the wave stores group g: its sum where the group is present, zero where it is not (unless accumulating)
  double v = 0.0;
  bool present = false;
#pragma unroll
  for (int q = 0; q < NGB; ++q) {
    if (DIRECT ? (int)((win.mask >> q) & 1ull) : (int)(q < win.np)) {        // (uniform)
      const double sum = clim_butterfly(a[q], 64);
      if ((DIRECT ? q : win.pg[q]) == lane) v = sum, present = true;
    }
  }
  if (lane < win.ng && (present || !accumulate)) {
    double* o = acc + row * win.ng + lane;
    *o = accumulate ? *o + v : v;
  }
}

// grid (ceil(rows / rpw), nf), rpw * 64 lanes, rpw * ng * 512 bytes of dynamic LDS: a wave per row, any number of
// groups.  Lane l keeps its accumulator of group g in LDS, at slot [g][l] of the wave's own image, instead of in a
// register: one read-modify-write per element whatever the number of groups (the lanes of a wave touch 64 consecutive
// doubles of one or more groups' slots, no bank conflict).  The order is that of the register form: lane l takes the
// times l + 64 i, i ascending.  The 64 partial sums of a group are then added in the order of the butterfly, as lane 0
// of it sees them -- (l, l + 32), then (l, l + 16) ... (0, 1) -- by all lanes over all groups at once, so the bits are
// those of time_sum_groups_long_kernel.  Nothing here crosses waves: no workgroup barrier.
template <typename T>
__global__ void __launch_bounds__(CLIM_THREADS)
time_sum_groups_long_lds_kernel(ClimPtrs fp, int64_t rows, int64_t nt, int64_t t0, GclimTab tb, GclimWindow win, int accumulate,
                                int rpw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gclim_dyn[];
  const int f = blockIdx.y;
  const void* srcv = nullptr;
  double* acc = nullptr;
#pragma unroll
  for (int q = 0; q < CLIM_NFMAX; ++q)
    if (q == f) srcv = fp.src[q], acc = fp.acc[q];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * rpw + wave;
  if (row >= rows) return;   // (uniform per wave)
  const int ng = win.ng;
  double* my = reinterpret_cast<double*>(gclim_dyn) + (size_t)wave * ng * 64;   // [ng][64]
  for (int g = 0; g < ng; ++g) my[g * 64 + lane] = -0.0;
  const T* __restrict__ p = reinterpret_cast<const T*>(srcv) + row * nt;
  const int32_t* __restrict__ lab = tb.lab + t0;
  const double* __restrict__ w = tb.w + t0;
  for (int64_t t = lane; t < nt; t += 256) {
    // (loads first: four in flight per lane; a time beyond the row carries the label of no group)
    const bool k1 = t + 64 < nt, k2 = t + 128 < nt, k3 = t + 192 < nt;
    const T x0 = p[t];
    const T x1 = k1 ? p[t + 64] : (T)0;
    const T x2 = k2 ? p[t + 128] : (T)0;
    const T x3 = k3 ? p[t + 192] : (T)0;
    const int l0 = lab[t];
    const int l1 = k1 ? lab[t + 64] : -1;
    const int l2 = k2 ? lab[t + 128] : -1;
    const int l3 = k3 ? lab[t + 192] : -1;
    const double w0 = w[t];
    const double w1 = k1 ? w[t + 64] : 0.0;
    const double w2 = k2 ? w[t + 128] : 0.0;
    const double w3 = k3 ? w[t + 192] : 0.0;
    if (l0 >= 0) my[l0 * 64 + lane] = __builtin_fma(w0, (double)x0, my[l0 * 64 + lane]);
    if (l1 >= 0) my[l1 * 64 + lane] = __builtin_fma(w1, (double)x1, my[l1 * 64 + lane]);
    if (l2 >= 0) my[l2 * 64 + lane] = __builtin_fma(w2, (double)x2, my[l2 * 64 + lane]);
    if (l3 >= 0) my[l3 * 64 + lane] = __builtin_fma(w3, (double)x3, my[l3 * 64 + lane]);
  }
  // ---- the 64 partial sums of every group, in the butterfly's order; the wave's LDS accesses complete in order ----
  for (int h = 32; h > 0; h >>= 1) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n = ng * h;
    for (int e = lane; e < n; e += 64) {
      const int g = e / h, l = e - g * h;
      double* s = my + g * 64 + l;
      s[0] = s[0] + s[h];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // lane g of the wave stores group g: its sum where the group is present, zero where it is not (unless accumulating)
  if (lane < ng) {
    const bool present = (win.mask >> lane) & 1ull;
    if (present || !accumulate) {
      const double v = present ? my[lane * 64] : 0.0;
      double* o = acc + row * ng + lane;
      *o = accumulate ? *o + v : v;
    }
  }
}

}  // namespace temx
