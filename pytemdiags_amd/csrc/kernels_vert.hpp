// kernels_vert.hpp -- vertical interpolation of model-level fields to pressure levels (include/temx_vert.h).
//
// NF fields [ncol][nlev][nt] -> [ncol][nplev][nt], time fastest, fp64 or fp32, no copy or re-layout of the fields.
// Source pressure of level k at (column i, time t):
//   hybrid   p = hyam[k] p0 + hybm[k] ps[i][t]   (fp64, two rounded products and one rounded sum, as numpy forms it)
//   field    p = P[i][k][t]
// Model levels are top first (p increases with k); the targets pt[j] are strictly ascending.
//
// One MERGE WALK per (column, time): k and the target index j advance together, the previous and the current level
// of all NF fields are held in registers, and every target with p_{k-1} < pt[j] <= p_k (>= p_0 on the first
// bracket) is emitted for all fields: value = y_{k-1} + w (y_k - y_{k-1}), w = (x - x_{k-1}) / (x_k - x_{k-1}) in fp64
// with x = ln p (log) or p (linear), rounded once to the field type.  The bracket search, the logarithms (taken only
// for brackets that hold a target) and the weights are shared by the NF fields.  Targets above p_0 / below p_bot
// follow the edge policy; a (column, time) whose pressures are not finite and strictly increasing (log: or not all
// positive) is NaN throughout.
//
// Two lane maps, neither of which puts the 64 lanes of a wave into 64 different rows:
//   vert_time_kernel  lanes run along time (then on into the next column): a wave reads ceil(64 / nt) + 1 row
//                     segments of nt elements per level.  For rows of nt * sizeof(T) >= 128 B.
//   vert_slab_kernel  for short rows.  The [nlev][nt] blocks of a run of columns are one contiguous span: a workgroup
//                     loads the spans of its columns with 16-byte coalesced loads into LDS (columns padded to an odd
//                     stride: lanes in neighbouring columns hit different banks), walks from LDS -- the levels of one
//                     (column, time) cut into SEG-bracket segments, one lane each, so that the few walks that fit in
//                     LDS still fill the workgroup -- and writes the output span back as one contiguous run.
#pragma once
#include "kernels.hpp"
#include "shared_defs.hpp"

namespace temx {

constexpr int VERT_NFMAX = 8;

template <int NF>
struct VertPtrs {
  const void* src[NF];
  void* dst[NF];
};

// device tables of one call: hyam[nlev], hybm[nlev] (hybrid only), pt[nplev] in Pa, xt[nplev] = ln pt or pt
struct VertTab {
  const double* hyam;
  const double* hybm;
  const double* pt;
  const double* xt;
};

__device__ __forceinline__ double vert_load_p(const void* p, int64_t idx, int p_f32) {
  return p_f32 ? (double)static_cast<const float*>(p)[idx] : static_cast<const double*>(p)[idx];
}

__device__ __forceinline__ double vert_hybrid_p(const VertTab& tb, int k, double p0, double ps) {
  return __dadd_rn(__dmul_rn(tb.hyam[k], p0), __dmul_rn(tb.hybm[k], ps));   // no fused multiply-add: numpy has none
}

// The merge walk over the levels k0..k1 of one (column, time).  first / last: this walk owns the targets above the
// top level / below the bottom level (a walk over the whole column has both).  A walk that is not the first skips
// the targets at or above its first level: the walk before it emits them.  pres(k) -> fp64 pressure, load(k, v) fills
// the NF values of level k, emit(j, f, value) stores one result.  Returns true when the pressures seen are not finite
// and strictly increasing, or (logp) the first of them is not positive (the caller then overwrites the column with NaN).
template <int NF, class PRES, class LOAD, class EMIT>
__device__ __forceinline__ bool vert_walk(int nf, int k0, int k1, bool first, bool last, int nplev, const VertTab& tb,
                                          bool logp, bool hold, double psurf, PRES pres, LOAD load, EMIT emit) {
  const double qnan = __builtin_nan("");
  double vp[NF], vc[NF], vn[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) vp[f] = vc[f] = vn[f] = 0.0;
  double pp = pres(k0);
  load(k0, vp);
  bool bad = !isfinite(pp) || (logp && !(pp > 0.0));   // ln p needs p > 0; the levels after the first must increase
  int j = 0;
  if (first) {
    for (; j < nplev && tb.pt[j] < pp; ++j)
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (f < nf) emit(j, f, hold ? vp[f] : qnan);
  } else {   // the first target below this walk's first level (a tie on that level belongs to the walk before)
    int hi = nplev;
    while (j < hi) {
      const int mid = (j + hi) >> 1;
      if (tb.pt[mid] <= pp) j = mid + 1;
      else hi = mid;
    }
  }
  // the next target stays in a register; NaN once the targets are used up (it compares false with everything)
  double ptj = j < nplev ? tb.pt[j] : qnan;
  double pn = pres(k0 + 1);
  load(k0 + 1, vn);
  for (int k = k0 + 1; k <= k1; ++k) {
    const double pc = pn;
#pragma unroll
    for (int f = 0; f < NF; ++f) vc[f] = vn[f];
    if (k < k1) {   // the next level is in flight while this bracket is worked on
      pn = pres(k + 1);
      load(k + 1, vn);
    }
    bad |= !(pc > pp) || !isfinite(pc);
    if (ptj <= pc) {
      const double x0 = logp ? log(pp) : pp, x1 = logp ? log(pc) : pc;
      const double dx = x1 - x0;
      do {
        const double w = (tb.xt[j] - x0) / dx;
#pragma unroll
        for (int f = 0; f < NF; ++f)
          if (f < nf) emit(j, f, vp[f] + w * (vc[f] - vp[f]));
        ++j;
        ptj = j < nplev ? tb.pt[j] : qnan;
      } while (ptj <= pc);
    }
    pp = pc;
#pragma unroll
    for (int f = 0; f < NF; ++f) vp[f] = vc[f];
  }
  if (last) {
    bad |= !isfinite(psurf);
    for (; j < nplev; ++j) {
      const bool h = hold && tb.pt[j] <= psurf;   // between the bottom level and the surface
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (f < nf) emit(j, f, h ? vp[f] : qnan);
    }
  }
  return bad;
}

// ---- lanes along time ------------------------------------------------------------------------------------------------
template <typename T, int NF, bool HYB>
__global__ void __launch_bounds__(VERT_THREADS)
vert_time_kernel(VertPtrs<NF> fp, int nf, int64_t ncol, int nlev, int64_t nt, int nplev, VertTab tb, double p0,
                 const void* __restrict__ P, int p_f32, int logp, int hold) {
  const int64_t g = blockIdx.x * (int64_t)VERT_THREADS + threadIdx.x;
  if (g >= ncol * nt) return;
  const int64_t i = g / nt, t = g - i * nt;
  const int64_t in0 = i * nlev * nt + t, out0 = i * nplev * nt + t;
  double ps = 0.0;
  if (HYB) ps = vert_load_p(P, g, p_f32);
  auto pres = [&](int k) { return HYB ? vert_hybrid_p(tb, k, p0, ps) : vert_load_p(P, in0 + k * nt, p_f32); };
  auto load = [&](int k, double* v) {
#pragma unroll
    for (int f = 0; f < NF; ++f)
      if (f < nf) v[f] = (double)static_cast<const T*>(fp.src[f])[in0 + k * nt];
  };
  auto emit = [&](int j, int f, double val) { static_cast<T*>(fp.dst[f])[out0 + j * nt] = (T)val; };
  const double psurf = HYB ? ps : pres(nlev - 1);
  const bool bad = vert_walk<NF>(nf, 0, nlev - 1, true, true, nplev, tb, logp != 0, hold != 0, psurf, pres, load, emit);
  if (bad)
    for (int j = 0; j < nplev; ++j)
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (f < nf) emit(j, f, __builtin_nan(""));
}

// ---- slab staged ---------------------------------------------------------------------------------------------------
// n elements of a contiguous global span <-> LDS, where the span is a run of columns of colsz elements and the LDS
// image gives each column `stride` elements.  16-byte global accesses over the aligned body of the span, single
// elements at its ends; g must be aligned to sizeof(E).
template <typename E>
__device__ __forceinline__ void vert_span_in(const E* __restrict__ g, E* s, int n, int colsz, int stride) {
  constexpr int V = 16 / (int)sizeof(E);
  const int tid = threadIdx.x;
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) / sizeof(E));
  if (head > n) head = n;
  const int nv = (n - head) / V, tail0 = head + nv * V;
  for (int e = tid; e < head + (n - tail0); e += VERT_THREADS) {
    const int ee = e < head ? e : tail0 + (e - head);
    const int col = ee / colsz;
    s[col * stride + (ee - col * colsz)] = g[ee];
  }
  for (int v = tid; v < nv; v += VERT_THREADS) {
    const int e0 = head + v * V;
    const float4 raw = *reinterpret_cast<const float4*>(g + e0);
    E tmp[V];
    __builtin_memcpy(tmp, &raw, 16);
    int col = e0 / colsz, r = e0 - col * colsz;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (r == colsz) {
        r = 0;
        ++col;
      }
      s[col * stride + r] = tmp[q];
      ++r;
    }
  }
}

template <typename E>
__device__ __forceinline__ void vert_span_out(E* __restrict__ g, const E* s, int n, int colsz, int stride) {
  constexpr int V = 16 / (int)sizeof(E);
  const int tid = threadIdx.x;
  int head = (int)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) / sizeof(E));
  if (head > n) head = n;
  const int nv = (n - head) / V, tail0 = head + nv * V;
  for (int e = tid; e < head + (n - tail0); e += VERT_THREADS) {
    const int ee = e < head ? e : tail0 + (e - head);
    const int col = ee / colsz;
    g[ee] = s[col * stride + (ee - col * colsz)];
  }
  for (int v = tid; v < nv; v += VERT_THREADS) {
    const int e0 = head + v * V;
    E tmp[V];
    int col = e0 / colsz, r = e0 - col * colsz;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (r == colsz) {
        r = 0;
        ++col;
      }
      tmp[q] = s[col * stride + r];
      ++r;
    }
    float4 raw;
    __builtin_memcpy(&raw, tmp, 16);
    *reinterpret_cast<float4*>(g + e0) = raw;
  }
}

// LDS of a workgroup: VertSlab (shared_defs.hpp), filled in by vert_slab_shape (launch_shapes.hpp)

template <typename T, int NF, bool HYB>
__global__ void __launch_bounds__(VERT_THREADS)
vert_slab_kernel(VertPtrs<NF> fp, int nf, int64_t ncol, int nlev, int nt, int nplev, VertTab tb, double p0,
                 const void* __restrict__ P, int p_f32, int logp, int hold, VertSlab sh) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vert_lds[];
  int* sbad = reinterpret_cast<int*>(vert_lds);
  unsigned char* base = vert_lds + VERT_THREADS * sizeof(int);
  unsigned char* sp = base;                                // the pressure image keeps the dtype of P
  T* s_in = reinterpret_cast<T*>(base + (HYB ? 0 : sh.p_img));
  T* s_out = reinterpret_cast<T*>(base + (HYB ? 0 : sh.p_img) + (size_t)nf * sh.in_img);
  const int in_per = sh.in_img / (int)sizeof(T), out_per = sh.out_img / (int)sizeof(T);

  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * sh.cw;
  const int ncw = (int)(ncol - c0 < sh.cw ? ncol - c0 : sh.cw);
  const int colsz = nlev * nt, ocolsz = nplev * nt;
  sbad[tid] = 0;
#pragma unroll
  for (int f = 0; f < NF; ++f)
    if (f < nf) vert_span_in(static_cast<const T*>(fp.src[f]) + c0 * colsz, s_in + f * in_per, ncw * colsz, colsz, sh.in_stride);
  if (!HYB) {
    if (p_f32) vert_span_in(static_cast<const float*>(P) + c0 * colsz, reinterpret_cast<float*>(sp), ncw * colsz, colsz, sh.in_stride);
    else vert_span_in(static_cast<const double*>(P) + c0 * colsz, reinterpret_cast<double*>(sp), ncw * colsz, colsz, sh.in_stride);
  }
  __syncthreads();

  // lane -> (segment, pair), pair fastest: the lanes of a wave work on the same levels of neighbouring columns
  const int npair = ncw * nt;
  const int pair = tid % (sh.cw * nt), s = tid / (sh.cw * nt);
  int bad = 0;
  if (pair < npair && s < sh.nseg) {
    const int c = pair / nt, t = pair - c * nt;
    const int k0 = s * sh.seg, k1 = min(k0 + sh.seg, nlev - 1);
    double ps = 0.0;
    if (HYB) ps = vert_load_p(P, c0 * nt + pair, p_f32);
    const int ib = c * sh.in_stride + t, ob = c * sh.out_stride + t;
    auto pres = [&](int k) {
      if (HYB) return vert_hybrid_p(tb, k, p0, ps);
      return p_f32 ? (double)reinterpret_cast<const float*>(sp)[ib + k * nt] : reinterpret_cast<const double*>(sp)[ib + k * nt];
    };
    auto load = [&](int k, double* v) {
#pragma unroll
      for (int f = 0; f < NF; ++f)
        if (f < nf) v[f] = (double)s_in[f * in_per + ib + k * nt];
    };
    auto emit = [&](int j, int f, double val) { s_out[f * out_per + ob + j * nt] = (T)val; };
    const double psurf = HYB ? ps : pres(nlev - 1);
    bad = vert_walk<NF>(nf, k0, k1, s == 0, k1 == nlev - 1, nplev, tb, logp != 0, hold != 0, psurf, pres, load, emit);
    if (bad) sbad[pair] = 1;   // every lane that sees it stores the same value
  }
  if (__syncthreads_or(bad)) {   // rare: some (column, time) of this workgroup is NaN throughout
    for (int pr = 0; pr < npair; ++pr) {
      if (!sbad[pr]) continue;   // same for every lane
      const int c = pr / nt, t = pr - c * nt;
      for (int e = tid; e < nf * nplev; e += VERT_THREADS) {
        const int f = e / nplev, j = e - f * nplev;
        s_out[f * out_per + c * sh.out_stride + t + j * nt] = (T)__builtin_nan("");
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int f = 0; f < NF; ++f)
    if (f < nf) vert_span_out(static_cast<T*>(fp.dst[f]) + c0 * ocolsz, s_out + f * out_per, ncw * ocolsz, ocolsz, sh.out_stride);
}

}  // namespace temx
