// kernels_ingest.hpp -- time-major model-level records straight to pressure levels in the engine's layout
// (include/temx_ingest.h): the re-layout of kernels_layout.hpp and the hybrid-level walk of kernels_vert.hpp in one pass.
//
// NF sources [nt_src][nlev][ncol] (ncol fastest, fp64 or fp32 each) and ps [nt_src][ncol] -> NF destinations
// [ncol][nplev][ntb] (time fastest, one dtype T) for the time window t0 .. t0 + ntb.  Source pressure
// p = hyam[k] p0 + hybm[k] ps, formed by vert_hybrid_p; the walk is vert_walk, unchanged, so every result has the bits
// temxv_interp gives on the output of temxl_to_engine.
//
// One workgroup owns one TILE of TC columns x TT times (IngestTile, chosen by ingest_tile in launch_shapes.hpp) and
// all levels of it, which it takes in windows of KW brackets:
//   read side    a window is nf * (levels) * TT rows of TC consecutive columns.  The lanes of a wave run along the
//                columns (64 / TC rows per wave instruction when TC < 64), INGEST_BATCH rows are in flight per lane
//                before the first is stored to LDS.  ps goes the same way, once.
//   LDS          image[f][slot][c][t], a column every `stride` elements with stride odd, as the re-layout has it.
//                The slots are a ring of KW + 1 levels: level k lives in slot k mod (KW + 1), so the last level of a
//                window is still there as the first level of the next one -- no level is read from HBM twice.
//   walk         one lane per (column, time) pair, time fastest across lanes (a lane takes `ppl` pairs when the tile
//                has more than INGEST_THREADS of them), vert_walk over the window's levels with first / last set on
//                the first / last window; the `bad` flag of a pair is carried across the windows in a register.
//   write side   emit stores straight to global: the lanes of one column write the run of TT times of a target level.
// Tails in ncol, nlev, nplev and ntb are masked on both sides: no load outside the window, no store outside
// dst[f][0 .. ncol * nplev * ntb).  All global offsets are int64_t.  No atomics: two calls give the same bits.
#pragma once
#include "kernels_vert.hpp"
#include "shared_defs.hpp"

namespace temx {

constexpr int INGEST_NFMAX = 8;
constexpr int INGEST_BATCH = 4;   // rows in flight per lane on the read side

struct IngestPtrs {
  const void* src[INGEST_NFMAX];
  void* dst[INGEST_NFMAX];
};

template <typename T, int NF>
__global__ void __launch_bounds__(INGEST_THREADS)
ingest_kernel(IngestPtrs fp, int nf, unsigned src_f32, int64_t ncol, int nlev, int64_t t0, int64_t ntb, int nplev,
              VertTab tb, double p0, const void* __restrict__ ps, int ps_f32, int logp, int hold, IngestTile tl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ingest_lds[];
  const int TC = 1 << tl.tc_shift;
  const int img = TC * tl.stride;                       // elements of one (field, slot) image, and of the ps image
  double* s_ps = reinterpret_cast<double*>(ingest_lds);
  T* s = reinterpret_cast<T*>(ingest_lds + (size_t)img * sizeof(double));
  const int nslot = tl.kw + 1;

  // block -> (column tile fastest, time tile): neighbouring workgroups read neighbouring pieces of the same rows
  const int ct = (int)(blockIdx.x % (unsigned)tl.nct), ti = (int)(blockIdx.x / (unsigned)tl.nct);
  const int64_t c0 = (int64_t)ct * TC, tc0 = (int64_t)ti * tl.tt;
  const int ncv = (int)(ncol - c0 < TC ? ncol - c0 : TC);          // valid columns and times of the tile
  const int ttv = (int)(ntb - tc0 < tl.tt ? ntb - tc0 : tl.tt);
  const int64_t lev_stride = ncol, time_stride = (int64_t)nlev * ncol;

  const int tid = threadIdx.x;
  const int rc = tid & (TC - 1), rsub = tid >> tl.tc_shift, rstep = INGEST_THREADS >> tl.tc_shift;
  const bool cok = rc < ncv;
  for (int t = rsub; t < ttv; t += rstep)
    if (cok) s_ps[rc * tl.stride + t] = vert_load_p(ps, (t0 + tc0 + t) * ncol + c0 + rc, ps_f32);

  unsigned badmask = 0;   // bit q: pair q of this lane has pressures that are not finite and strictly increasing
  for (int w = 0; w < tl.nwin; ++w) {
    const int k0 = w * tl.kw, k1 = min(k0 + tl.kw, nlev - 1);
    const int s0 = k0 % nslot;                          // slot of level k0; level k sits in slot_of(k)
    auto slot_of = [&](int k) {
      const int sl = s0 + (k - k0);
      return sl >= nslot ? sl - nslot : sl;
    };
    const int ka = w == 0 ? k0 : k0 + 1, nk = k1 - ka + 1;   // level k0 of a later window is in the ring already
    __syncthreads();                                    // the walks of the window before are done with the slots
    // ---- read side ----
    const int nrow = nf * nk * ttv;
    for (int rb = rsub; rb < nrow; rb += rstep * INGEST_BATCH) {
      T v[INGEST_BATCH];
      int at[INGEST_BATCH];
#pragma unroll
      for (int q = 0; q < INGEST_BATCH; ++q) {
        const int r = rb + q * rstep;
        v[q] = (T)0;
        at[q] = -1;
        if (cok && r < nrow) {
          const int x = r / ttv, t = r - x * ttv;
          const int f = x / nk, k = ka + (x - f * nk);
          const void* srcv = nullptr;
#pragma unroll
          for (int g = 0; g < INGEST_NFMAX; ++g)
            if (g == f) srcv = fp.src[g];
          const int64_t off = (t0 + tc0 + t) * time_stride + (int64_t)k * lev_stride + c0 + rc;
          const bool f32 = sizeof(T) == 4 || ((src_f32 >> f) & 1u);
          v[q] = f32 ? (T) static_cast<const float*>(srcv)[off] : (T) static_cast<const double*>(srcv)[off];
          at[q] = (f * nslot + slot_of(k)) * img + rc * tl.stride + t;
        }
      }
#pragma unroll
      for (int q = 0; q < INGEST_BATCH; ++q)
        if (at[q] >= 0) s[at[q]] = v[q];
    }
    __syncthreads();
    // ---- walk: pair = c * tt + t, time fastest across the lanes ----
    for (int q = 0; q < tl.ppl; ++q) {
      const int pair = tid + q * INGEST_THREADS;
      const int c = pair / tl.tt, t = pair - c * tl.tt;
      if (c >= ncv || t >= ttv) continue;
      const int ib = c * tl.stride + t;
      const double psv = s_ps[ib];
      const int64_t ob = (c0 + c) * (int64_t)nplev * ntb + tc0 + t;
      auto pres = [&](int k) { return vert_hybrid_p(tb, k, p0, psv); };
      auto load = [&](int k, double* v) {
        const int sl = slot_of(k);
#pragma unroll
        for (int f = 0; f < NF; ++f)
          if (f < nf) v[f] = (double)s[(f * nslot + sl) * img + ib];
      };
      auto emit = [&](int j, int f, double val) { static_cast<T*>(fp.dst[f])[ob + (int64_t)j * ntb] = (T)val; };
      const bool bad = vert_walk<NF>(nf, k0, k1, w == 0, k1 == nlev - 1, nplev, tb, logp != 0, hold != 0, psv, pres,
                                     load, emit);
      if (bad) badmask |= 1u << q;
    }
  }
  if (badmask) {   // rare: the pair is NaN throughout (its own stores above are ordered before these)
    for (int q = 0; q < tl.ppl; ++q) {
      if (!((badmask >> q) & 1u)) continue;
      const int pair = tid + q * INGEST_THREADS;
      const int c = pair / tl.tt, t = pair - c * tl.tt;
      const int64_t ob = (c0 + c) * (int64_t)nplev * ntb + tc0 + t;
      for (int j = 0; j < nplev; ++j)
#pragma unroll
        for (int f = 0; f < NF; ++f)
          if (f < nf) static_cast<T*>(fp.dst[f])[ob + (int64_t)j * ntb] = (T)__builtin_nan("");
    }
  }
}

}  // namespace temx
