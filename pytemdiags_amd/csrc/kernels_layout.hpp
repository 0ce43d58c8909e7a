// kernels_layout.hpp -- time-major records to the engine's layout (include/temx_layout.h).
//
// NF sources [nt_src][nlev][ncol] (ncol fastest, fp64 or fp32 each) -> NF destinations [ncol][nlev][ntb] (time
// fastest, one dtype), for the time window t0 .. t0 + ntb; optionally with the level order reversed.  Every element is
// read once and written once; a move between equal dtypes carries the bits (the LDS image is unsigned words).
//
// One workgroup moves one TILE of one field: TC columns x KL destination levels x TT times.
//   read side    the tile is KL * TT rows of TC consecutive columns.  The lanes of a wave run along the columns (two
//                rows per wave instruction when TC = 32), LAYOUT_BATCH rows are in flight per wave before the first is
//                stored to LDS.
//   LDS          image[c][r], r = kl * TT + tt, a column every `stride` elements with stride odd: on the read side the
//                lanes of a store group (16 lanes of ds_write_b64, 32 of ds_write_b32) fall into different banks, on
//                the write side the lanes of a wave read consecutive words.
//   write side   the r-range of one column is ONE contiguous run of the destination: the host (layout_tile) picks
//                either TT = ntb, where the rows of KL neighbouring levels follow each other (run = KL * ntb elements,
//                as ntb alone is a short run), or KL = 1 with TT a chunk of a long time axis.  A wave writes the run of
//                one column at a time, lanes along the run.
// Tails in ncol, nlev and ntb are masked on both sides: no load outside the window, no store outside
// dst[f][0 .. ncol * nlev * ntb).  All global offsets are int64_t.
#pragma once
#include "kernels.hpp"
#include "shared_defs.hpp"

namespace temx {

constexpr int LAYOUT_NFMAX = 8;
constexpr int LAYOUT_THREADS = 256;
constexpr int LAYOUT_BATCH = 4;          // rows in flight per wave on the read side
constexpr int LAYOUT_LDS_BYTES = 33 * 1024;   // per workgroup: a 32 KiB tile plus the padding of its columns

struct LayoutPtrs {
  const void* src[LAYOUT_NFMAX];
  void* dst[LAYOUT_NFMAX];
};

// tile of a launch: LayoutTile (shared_defs.hpp), chosen by layout_tile (launch_shapes.hpp)

template <typename U>
struct LayoutWide;   // the narrower source of U, if there is one
template <>
struct LayoutWide<uint64_t> {
  static __device__ __forceinline__ uint64_t widen(float v) { return (uint64_t)__double_as_longlong((double)v); }
};
template <>
struct LayoutWide<uint32_t> {
  static __device__ __forceinline__ uint32_t widen(float v) { return __float_as_uint(v); }   // never taken: fp32 -> fp32 is a bit copy
};

// U: unsigned word of the destination dtype (uint64_t fp64, uint32_t fp32).  src_f32: bit f set = source f is fp32.
template <typename U>
__global__ void __launch_bounds__(LAYOUT_THREADS)
layout_to_engine_kernel(LayoutPtrs fp, int nf, unsigned src_f32, int64_t ncol, int nlev, int64_t t0, int64_t ntb,
                        int flip, LayoutTile tl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char layout_lds[];
  U* s = reinterpret_cast<U*>(layout_lds);

  // block -> (column tile fastest, field, level tile, time tile): neighbouring workgroups read neighbouring pieces
  // of the same source rows
  unsigned b = blockIdx.x;
  const int ct = (int)(b % (unsigned)tl.nct);
  b /= (unsigned)tl.nct;
  const int f = (int)(b % (unsigned)nf);
  b /= (unsigned)nf;
  const int lt = (int)(b % (unsigned)tl.nlt);
  const int tt_i = (int)(b / (unsigned)tl.nlt);
  if (tt_i >= tl.ntt) return;   // (uniform; the host launches exactly nct * nf * nlt * ntt workgroups)

  const void* srcv = nullptr;
  void* dstv = nullptr;
#pragma unroll
  for (int g = 0; g < LAYOUT_NFMAX; ++g)
    if (g == f) srcv = fp.src[g], dstv = fp.dst[g];
  const bool f32 = sizeof(U) == 4 || ((src_f32 >> f) & 1u);

  const int TC = 1 << tl.tc_shift;
  const int64_t c0 = (int64_t)ct * TC;
  const int k0 = lt * tl.kl;                                   // first destination level of the tile
  const int64_t tc0 = (int64_t)tt_i * tl.tt;                   // first time of the tile inside the window
  const int ncv = (int)(ncol - c0 < TC ? ncol - c0 : TC);      // valid columns, levels, times
  const int klv = nlev - k0 < tl.kl ? nlev - k0 : tl.kl;
  const int ttv = (int)(ntb - tc0 < tl.tt ? ntb - tc0 : tl.tt);
  const int nrow = klv * ttv;   // (ttv == tl.tt whenever klv > 1: the rows r = kl * tt + t of the tile are 0 .. nrow)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- read side ----
  {
    const int c = lane & (TC - 1), rsub = lane >> tl.tc_shift;   // rsub 0 (TC = 64) or 0..1 (TC = 32)
    const int rpw = 64 >> tl.tc_shift;                           // rows per wave instruction
    const int rstep = rpw * (LAYOUT_THREADS / 64);
    const bool cok = c < ncv;
    const int64_t lev_stride = ncol, time_stride = (int64_t)nlev * ncol;
    for (int rb = wave * rpw + rsub; rb < nrow; rb += rstep * LAYOUT_BATCH) {
      U v[LAYOUT_BATCH];
#pragma unroll
      for (int q = 0; q < LAYOUT_BATCH; ++q) {
        const int r = rb + q * rstep;
        v[q] = 0;
        if (cok && r < nrow) {
          const int kl = r / ttv, t = r - kl * ttv;
          const int kd = k0 + kl, ks = flip ? nlev - 1 - kd : kd;
          const int64_t off = (t0 + tc0 + t) * time_stride + (int64_t)ks * lev_stride + c0 + c;
          if (sizeof(U) == 4) v[q] = (U) reinterpret_cast<const uint32_t*>(srcv)[off];
          else if (f32) v[q] = LayoutWide<U>::widen(reinterpret_cast<const float*>(srcv)[off]);
          else v[q] = (U) reinterpret_cast<const uint64_t*>(srcv)[off];
        }
      }
#pragma unroll
      for (int q = 0; q < LAYOUT_BATCH; ++q) {
        const int r = rb + q * rstep;
        if (cok && r < nrow) s[c * tl.stride + r] = v[q];
      }
    }
  }
  __syncthreads();
  // ---- write side: rows 0 .. nrow of a column are one run of the destination ----
  {
    const int64_t col_stride = (int64_t)nlev * ntb;
    const int64_t run0 = (int64_t)k0 * ntb + tc0;
    U* d = reinterpret_cast<U*>(dstv);
    for (int c = wave; c < ncv; c += LAYOUT_THREADS / 64) {
      U* dc = d + (c0 + c) * col_stride + run0;
      const U* sc = s + c * tl.stride;
      for (int r = lane; r < nrow; r += 64) dc[r] = sc[r];
    }
  }
}

}  // namespace temx
