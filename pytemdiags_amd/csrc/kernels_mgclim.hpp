// kernels_mgclim.hpp -- the grouped, weighted sum over the valid times of fields with missing values
// (../include/temx_mgclim.h, temxw_time_sum_groups_valid).
//
// NF sources [ncol][nlev][nt] (one block of a record, time fastest, one dtype for the call) -> per field the fp64 sums
// of w * x over the valid times of each group, the sums of their weights and their number, [ncol][nlev][ng] each.  An
// element is valid iff it is finite (nclim_valid: the exponent bits); under a common mask a time of a row is valid iff
// it is valid in every field.  fp32 widens exactly; every step of a sum is one fp64 fma a <- w * x + a, of a weight sum
// a <- a + w; a value that is not valid enters no arithmetic.  The kernels are those of kernels_gclim.hpp with the NFT
// fields of a workgroup (kernels_nclim.hpp: 1 in own-mask mode, the fields along blockIdx.y; 4 or 8 under a common mask)
// and the validity test; mgclim_shapes.hpp cuts the launch, and the order of the additions of a (row, group) is that of
// temxg_time_sum_groups at the same (nt, dtype):
//   staged    (time_sum_groups_valid_staged_kernel) the nfs images of the workgroup's rows lie in LDS (nclim_stage, all
//             fields before one barrier).  A unit is (group present, row), packed densely over the 256 lanes: unit
//             u = (u / nr, u % nr), so the lanes of a wave read one time of neighbouring rows (odd stride: different
//             banks) and a wave may straddle two groups.  The window's entries of the sorted table (time, weight) are
//             copied to LDS next to the rows, group after group (6 KiB more: four workgroups per CU).  A lane walks
//             its group's times in ascending order with one accumulator per output and stores nfs + 2 values.
//   long row, registers  (time_sum_groups_valid_long_kernel<T, NFT, NGB>) a wave per row, the nfs values of four times
//             per lane in flight; NGB * (nfs + 1) fp64 accumulators and NGB counts; label == g && ok ? fma : keep; one
//             butterfly per (group present, output); lane g stores group g.
//   long row, LDS  (time_sum_groups_valid_long_lds_kernel<T, NFT>) the accumulators of lane l live at
//             [slot][output][l] of the wave's own image, a slot per group present of the current batch; one
//             read-modify-write per valid element and output; then the 64 partial sums of every (slot, output) are
//             added in the butterfly's order by all lanes at once.  One walk of the row per batch of groups present.
// Sums start from -0.0.  Without `accumulate` the groups absent from the block are stored as zero; with it they are
// neither read nor written.  Each output is stored once, by one lane; nothing else is written.  All global offsets are
// int64_t.
#pragma once
#include "kernels_gclim.hpp"
#include "kernels_nclim.hpp"
#include "mgclim_shapes.hpp"
#include <hip/hip_runtime.h>

#include <cstdint>

namespace temx {

struct MgclimPtrs {
  const void* src[MGCLIM_NFMAX];
  double* acc[MGCLIM_NFMAX];
  double* wsum[MGCLIM_NFMAX];   // common-mask mode: [0] only
  double* cnt[MGCLIM_NFMAX];    // common-mask mode: [0] only
};

// the pointers of a workgroup: field blockIdx.y alone (NFT = 1) or the first NFT fields
template <int NFT>
__device__ __forceinline__ void mgclim_select(const MgclimPtrs& fp, const void* (&src)[NFT], double* (&acc)[NFT],
                                              double*& wsum, double*& cnt) {
  if (NFT == 1) {
    const int f = blockIdx.y;
    src[0] = nullptr, acc[0] = nullptr, wsum = nullptr, cnt = nullptr;
#pragma unroll
    for (int q = 0; q < MGCLIM_NFMAX; ++q)
      if (q == f) src[0] = fp.src[q], acc[0] = fp.acc[q], wsum = fp.wsum[q], cnt = fp.cnt[q];
  } else {
#pragma unroll
    for (int q = 0; q < NFT; ++q) src[q] = fp.src[q], acc[q] = fp.acc[q];
    wsum = fp.wsum[0], cnt = fp.cnt[0];
  }
}

// the number of groups present below g: the slot of a present group g
__device__ __forceinline__ int mgclim_rank(unsigned long long mask, int g) {
  return __popcll(mask & ((1ull << g) - 1ull));
}

// grid (ceil(rows / rpb), NFT == 1 ? nf : 1); nfs * rpb * stride * sizeof(T) <= NCLIM_LDS_BYTES; nt < MGCLIM_STAGED_NT
template <typename T, int NFT>
__global__ void __launch_bounds__(MGCLIM_THREADS)
time_sum_groups_valid_staged_kernel(MgclimPtrs fp, int nf, int64_t rows, int nt, int t0, int rpb, int stride, GclimTab tb,
                                    GclimWindow win, int accumulate) {
  __shared__ __attribute__((aligned(16))) unsigned char mgclim_lds[NCLIM_LDS_BYTES];
  __shared__ double tab_w[MGCLIM_STAGED_NT];   // the window's table entries, group after group: weights ...
  __shared__ int tab_t[MGCLIM_STAGED_NT];      // ... and times inside the block, ascending within a group
  const void* srcv[NFT];
  double* acc[NFT];
  double *wsum, *cnt;
  mgclim_select<NFT>(fp, srcv, acc, wsum, cnt);
  const int nfs = NFT == 1 ? 1 : nf;                       // fields of this workgroup
  const int img = rpb * stride;                            // elements of one field's image
  T* s = reinterpret_cast<T*>(mgclim_lds);
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  if (r0 >= rows) return;   // (uniform; the host launches exactly ceil(rows / rpb) workgroups along x)
  const int nr = (int)(rows - r0 < rpb ? rows - r0 : rpb);        // valid rows of this workgroup
  const int tid = threadIdx.x;
  // the table entries of the window go to LDS with the rows (at most nt of them): a unit's walk is a serial chain, and
  // with few rows per workgroup nothing hides the latency of a global load per step
  for (int q = 0, off = 0; q < win.np; ++q) {       // (uniform)
    const int lo = win.lo[q], n = win.hi[q] - lo;
    for (int k = tid; k < n; k += MGCLIM_THREADS) tab_t[off + k] = tb.st[lo + k] - t0, tab_w[off + k] = tb.sw[lo + k];
    off += n;
  }
#pragma unroll
  for (int f = 0; f < NFT; ++f)
    if (f < nfs) nclim_stage<T>(reinterpret_cast<const T*>(srcv[f]) + r0 * nt, s + f * img, nr * nt, nt, stride, tid);
  __syncthreads();

  // ---- sum side: unit = (group present, row), dense over the lanes ----
  const int ng = win.ng;
  const int units = win.np * nr;
  for (int u = tid; u < units; u += MGCLIM_THREADS) {
    const int q = u / nr, r = u - q * nr;
    const int g = win.pg[q];
    int lo = 0;                                      // the group's entries in the LDS table: those before it, then its own
    for (int p = 0; p < q; ++p) lo += win.hi[p] - win.lo[p];
    const int hi = lo + win.hi[q] - win.lo[q];
    const T* sr = s + r * stride;
    double a[NFT];
#pragma unroll
    for (int f = 0; f < NFT; ++f) a[f] = -0.0;
    double ws = -0.0;
    int c = 0;
    for (int j = lo; j < hi; ++j) {
      const int t = tab_t[j];
      const double w = tab_w[j];
      T x[NFT];
      bool ok = true;
#pragma unroll
      for (int f = 0; f < NFT; ++f)
        if (f < nfs) x[f] = sr[f * img + t], ok = ok && nclim_valid(x[f]);
      if (ok) {
#pragma unroll
        for (int f = 0; f < NFT; ++f)
          if (f < nfs) a[f] = __builtin_fma(w, (double)x[f], a[f]);
        ws = ws + w;
        ++c;
      }
    }
    const int64_t o = (r0 + r) * ng + g;
#pragma unroll
    for (int f = 0; f < NFT; ++f)
      if (f < nfs) acc[f][o] = accumulate ? acc[f][o] + a[f] : a[f];
    wsum[o] = accumulate ? wsum[o] + ws : ws;
    cnt[o] = accumulate ? cnt[o] + (double)c : (double)c;
  }
  // the groups absent from the block: zero, unless the call accumulates
  if (!accumulate && win.np < ng) {
    const int n = nr * ng;
    for (int e = tid; e < n; e += MGCLIM_THREADS) {
      const int g = e % ng;
      if (!((win.mask >> g) & 1ull)) {
        const int64_t o = r0 * ng + e;
#pragma unroll
        for (int f = 0; f < NFT; ++f)
          if (f < nfs) acc[f][o] = 0.0;
        wsum[o] = 0.0;
        cnt[o] = 0.0;
      }
    }
  }
}

// grid (ceil(rows / NCLIM_LONG_ROWS), NFT == 1 ? nf : 1): a wave per row, at most NGB groups present in the block
template <typename T, int NFT, int NGB>
__global__ void __launch_bounds__(MGCLIM_THREADS)
time_sum_groups_valid_long_kernel(MgclimPtrs fp, int nf, int64_t rows, int64_t nt, int64_t t0, GclimTab tb, GclimWindow win,
                                  int accumulate) {
  const void* srcv[NFT];
  double* acc[NFT];
  double *wsum, *cnt;
  mgclim_select<NFT>(fp, srcv, acc, wsum, cnt);
  const int nfs = NFT == 1 ? 1 : nf;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * NCLIM_LONG_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;   // (uniform per wave)
  const T* p[NFT];
#pragma unroll
  for (int f = 0; f < NFT; ++f) p[f] = reinterpret_cast<const T*>(srcv[f]) + row * nt;
  const int32_t* __restrict__ lab = tb.lab + t0;
  const double* __restrict__ w = tb.w + t0;
  int gq[NGB];               // the q-th group present (-2 beyond the groups present: matches no label)
#pragma unroll
  for (int q = 0; q < NGB; ++q) gq[q] = win.pg[q];
  double a[NGB][NFT], ws[NGB];
  int c[NGB];
#pragma unroll
  for (int q = 0; q < NGB; ++q) {
#pragma unroll
    for (int f = 0; f < NFT; ++f) a[q][f] = -0.0;
    ws[q] = -0.0, c[q] = 0;
  }
  for (int64_t t = lane; t < nt; t += 256) {
    // (loads first: four times of every field in flight per lane; a field beyond nfs reads nothing and counts as valid; a
    // time beyond the row carries the label of no group)
    T x[4][NFT];
    int l[4];
    double wt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool k = t + 64 * i < nt;
#pragma unroll
      for (int f = 0; f < NFT; ++f) x[i][f] = (k && f < nfs) ? p[f][t + 64 * i] : (T)0;
      l[i] = k ? lab[t + 64 * i] : -1;
      wt[i] = k ? w[t + 64 * i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bool ok = true;
#pragma unroll
      for (int f = 0; f < NFT; ++f) ok = ok && nclim_valid(x[i][f]);
#pragma unroll
      for (int q = 0; q < NGB; ++q) {
        const bool hit = ok && l[i] == gq[q];
#pragma unroll
        for (int f = 0; f < NFT; ++f) a[q][f] = hit ? __builtin_fma(wt[i], (double)x[i][f], a[q][f]) : a[q][f];
        ws[q] = hit ? ws[q] + wt[i] : ws[q];
        c[q] += hit ? 1 : 0;
      }
    }
  }
  // lane g of the wave stores group g: its sums where the group is present, zero where it is not (unless accumulating)
  double v[NFT], vw = 0.0, vc = 0.0;
#pragma unroll
  for (int f = 0; f < NFT; ++f) v[f] = 0.0;
  bool present = false;
#pragma unroll
  for (int q = 0; q < NGB; ++q) {
    if (q < win.np) {        // (uniform)
      const bool mine = gq[q] == lane;
#pragma unroll
      for (int f = 0; f < NFT; ++f)
        if (f < nfs) {
          const double sum = clim_butterfly(a[q][f], 64);
          if (mine) v[f] = sum;
        }
      const double sw = clim_butterfly(ws[q], 64);
      const int sc = nclim_butterfly(c[q], 64);
      if (mine) vw = sw, vc = (double)sc, present = true;
    }
  }
  if (lane < win.ng && (present || !accumulate)) {
    const int64_t o = row * win.ng + lane;
#pragma unroll
    for (int f = 0; f < NFT; ++f)
      if (f < nfs) acc[f][o] = accumulate ? acc[f][o] + v[f] : v[f];
    wsum[o] = accumulate ? wsum[o] + vw : vw;
    cnt[o] = accumulate ? cnt[o] + vc : vc;
  }
}

// grid (ceil(rows / rpw), NFT == 1 ? nf : 1), rpw * 64 lanes, rpw * batch * (nfs + 2) * 512 bytes of dynamic LDS: a wave
// per row, any number of groups present, `batch` of them per walk of the row.  The image of a wave is
// [slot][output][64 lanes] doubles: outputs 0 .. nfs-1 the sums of the fields, nfs the weights, nfs + 1 the count.
// Nothing here crosses waves: no workgroup barrier.
template <typename T, int NFT>
__global__ void __launch_bounds__(MGCLIM_THREADS)
time_sum_groups_valid_long_lds_kernel(MgclimPtrs fp, int nf, int64_t rows, int64_t nt, int64_t t0, GclimTab tb, GclimWindow win,
                                      int accumulate, int rpw, int batch) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mgclim_dyn[];
  const void* srcv[NFT];
  double* acc[NFT];
  double *wsum, *cnt;
  mgclim_select<NFT>(fp, srcv, acc, wsum, cnt);
  const int nfs = NFT == 1 ? 1 : nf;
  const int nout = nfs + 2;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * rpw + wave;
  if (row >= rows) return;   // (uniform per wave)
  const int ng = win.ng, np = win.np;
  const unsigned long long mask = win.mask;
  double* my = reinterpret_cast<double*>(mgclim_dyn) + (size_t)wave * batch * nout * 64;
  const T* p[NFT];
#pragma unroll
  for (int f = 0; f < NFT; ++f) p[f] = reinterpret_cast<const T*>(srcv[f]) + row * nt;
  const int32_t* __restrict__ lab = tb.lab + t0;
  const double* __restrict__ w = tb.w + t0;
  const int mygroup = lane < ng && ((mask >> lane) & 1ull) ? mgclim_rank(mask, lane) : -1;   // lane g: the slot of group g
  for (int b0 = 0; b0 < np; b0 += batch) {                  // the slots b0 .. b0 + nb of this pass
    const int nb = np - b0 < batch ? np - b0 : batch;
    for (int sl = 0; sl < nb; ++sl) {
      for (int o = 0; o <= nfs; ++o) my[(sl * nout + o) * 64 + lane] = -0.0;
      my[(sl * nout + nfs + 1) * 64 + lane] = 0.0;
    }
    for (int64_t t = lane; t < nt; t += 256) {
      // (loads first: four times of every field in flight per lane)
      T x[4][NFT];
      int l[4];
      double wt[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool k = t + 64 * i < nt;
#pragma unroll
        for (int f = 0; f < NFT; ++f) x[i][f] = (k && f < nfs) ? p[f][t + 64 * i] : (T)0;
        l[i] = k ? lab[t + 64 * i] : -1;
        wt[i] = k ? w[t + 64 * i] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bool ok = l[i] >= 0;
#pragma unroll
        for (int f = 0; f < NFT; ++f) ok = ok && nclim_valid(x[i][f]);
        const int sl = mgclim_rank(mask, l[i] & 63) - b0;
        if (ok && sl >= 0 && sl < nb) {
          double* m = my + sl * nout * 64 + lane;
#pragma unroll
          for (int f = 0; f < NFT; ++f)
            if (f < nfs) m[f * 64] = __builtin_fma(wt[i], (double)x[i][f], m[f * 64]);
          m[nfs * 64] = m[nfs * 64] + wt[i];
          m[(nfs + 1) * 64] = m[(nfs + 1) * 64] + 1.0;
        }
      }
    }
    // ---- the 64 partial sums of every (slot, output), in the butterfly's order; the wave's LDS accesses complete in order ----
    for (int h = 32; h > 0; h >>= 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const int n = nb * nout * h;
      for (int e = lane; e < n; e += 64) {
        const int u = e / h, k = e - u * h;
        double* sp = my + u * 64 + k;
        sp[0] = sp[0] + sp[h];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // lane g of the wave stores group g: its sums in the pass that holds its slot; zero where the group is absent, in the
    // first pass (unless accumulating)
    if (lane < ng) {
      const int sl = mygroup - b0;
      const bool here = mygroup >= 0 && sl >= 0 && sl < nb;
      if (here || (mygroup < 0 && b0 == 0 && !accumulate)) {
        const int64_t o = row * ng + lane;
        const double* m = my + (here ? sl : 0) * nout * 64;
#pragma unroll
        for (int f = 0; f < NFT; ++f)
          if (f < nfs) {
            const double v = here ? m[f * 64] : 0.0;
            acc[f][o] = accumulate ? acc[f][o] + v : v;
          }
        const double vw = here ? m[nfs * 64] : 0.0, vc = here ? m[(nfs + 1) * 64] : 0.0;
        wsum[o] = accumulate ? wsum[o] + vw : vw;
        cnt[o] = accumulate ? cnt[o] + vc : vc;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace temx
