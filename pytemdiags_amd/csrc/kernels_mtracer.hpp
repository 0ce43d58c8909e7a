// kernels_mtracer.hpp -- tracer TEM in missing-value mode (include/temx_mtracer.h): a tracer q with a mask of its own.
//
// A point (i, d) is valid for the tracer when q, v and omega are all finite there (the three arrays a tracer run
// reads).  qb is the masked fit of q under that mask -- the functional, tau, Q basis and product linearisation of
// kernels_miss.hpp -- and the products q'v', q'omega' are fitted under the same mask with the masked v, omega
// coefficients of the TEM run.  Kernels:
//   miss_tracer_project_kernel  one read of (q, v, omega): the tracer's mask, b for q (K rows) and e (2L+1 rows)
//   miss_tracer_native_kernel   the three native tracer fields qp, qpvp, qpwapp, NaN where not valid / thin
// The systems are miss_system_kernel<1> and <2> (kernels_miss.hpp), the masked products of the sweep are the KIND = 3
// instantiation of eddy_kernel (kernels.hpp), the epilogue is tracer_epilogue_kernel (kernels.hpp), all unchanged.
#pragma once
#include "kernels_miss.hpp"

namespace temx {

// partial[split][r][d], r < K: the select-projection of q on Q; then NE rows of the projection of the tracer's
// missing indicator on raw harmonics -- the layout of miss_project_kernel with NF = 1.
// Tiling and pipeline of project_kernel: one wave = one d-tile (16 columns), four waves per workgroup.  The rows of
// (q, v, omega) come from HBM straight into registers in the MFMA B layout, PD chunks ahead (a ring whose slot is
// re-loaded as soon as it has been consumed); the A blocks of a chunk -- TB blocks of Q and TBE raw-row blocks per
// group -- are staged through LDS by the whole workgroup, double buffered, one barrier per chunk.  Chunks whose rows
// all exist, and whose successors PD ahead do, take a path without row clamps or liveness tests.
// TB + TBE accumulators per lane (48 at K <= 64): two waves per SIMD.
template <typename T, int TB, int TBE, int PD>
__global__ void __launch_bounds__(256, 2)
miss_tracer_project_kernel(FieldPtrs<3> fp, int64_t N, int64_t D, int K, int NE, const double* __restrict__ yblk,
                           int gstride, const double* __restrict__ eblk, int64_t nchunk, double* __restrict__ partial,
                           int nsplit, int ndt) {
  static_assert(PD >= 1 && PD <= 3, "ring depth");
  constexpr int YA = 4 * TB * 16, EA = 4 * TBE * 16;   // doubles of A blocks per chunk
  constexpr int YJ = (YA + 255) / 256, EJ = (EA + 255) / 256;   // staging loads per thread
  __shared__ double stage[2][YA + EA];
  int split, dq;
  if (!wg_work((ndt + 3) / 4, nsplit, split, dq)) return;
  const int wave = uniform_wave();
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = lane & 15, g = lane >> 4;
  const int dt = dq * 4 + wave;
  const bool active = dt < ndt;                        // ragged last quad: helper waves only stage
  const int64_t d = (int64_t)dt * 16 + c;
  const bool dvalid = active && d < D;
  const int64_t dcl = d < D ? d : D - 1;
  const int c0 = (int)(nchunk * split / nsplit), c1 = (int)(nchunk * (split + 1) / nsplit);   // uniform

  const uint32_t loff = (uint32_t)(g * D + dcl);          // host guarantees 4*D < 2^31
  const uint32_t yoff = (uint32_t)(g * 4 + (lane & 3));   // A[i = lane&3 -> harmonic][k = lane>>4 -> row]
  const T* fb[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) fb[f] = reinterpret_cast<const T*>(fp.p[f]);

  double acc[TB], acce[TBE];
#pragma unroll
  for (int t = 0; t < TB; ++t) acc[t] = 0.0;
#pragma unroll
  for (int t = 0; t < TBE; ++t) acce[t] = 0.0;

  T xn[PD][3][4];
  double ys[YJ], es[EJ];
  const int nfull = (int)(N >> 4);           // chunks whose 16 rows all exist
  auto load_x = [&](int chunk, auto slotc, int ti, auto fastc) __attribute__((always_inline)) {
    constexpr int slot = decltype(slotc)::value;
    const int64_t gb = (int64_t)chunk * 16 + ti * 4;   // first row of the group (uniform)
    if (decltype(fastc)::value) {
#pragma unroll
      for (int f = 0; f < 3; ++f) xn[slot][f][ti] = (fb[f] + gb * D)[loff];
    } else {                                  // ragged tail of the grid: clamp per lane
      int64_t row = gb + g;
      row = row < N ? row : N - 1;
#pragma unroll
      for (int f = 0; f < 3; ++f) xn[slot][f][ti] = fb[f][row * D + dcl];
    }
  };
  // element tid + 256 j of a chunk's Q image = (group gi, block t, element e); in yblk the groups of a chunk are
  // gstride blocks apart.  The raw-row image of a chunk is contiguous in eblk.  Offsets past an image are clamped to
  // its first element (loaded, never stored).
  uint32_t yso[YJ], eso[EJ];
#pragma unroll
  for (int j = 0; j < YJ; ++j) {
    const int li = tid + 256 * j;
    const int gi = li / (TB * 16), rem = li % (TB * 16);
    yso[j] = li < YA ? (uint32_t)(gi * gstride * 16 + rem) : 0u;
  }
#pragma unroll
  for (int j = 0; j < EJ; ++j) eso[j] = tid + 256 * j < EA ? (uint32_t)(tid + 256 * j) : 0u;
  const int64_t ychunk = (int64_t)4 * gstride * 16;
  auto load_a = [&](int chunk) __attribute__((always_inline)) {   // chunk < nchunk: inside both arrays
#pragma unroll
    for (int j = 0; j < YJ; ++j) ys[j] = (yblk + (int64_t)chunk * ychunk)[yso[j]];
#pragma unroll
    for (int j = 0; j < EJ; ++j) es[j] = (eblk + (int64_t)chunk * EA)[eso[j]];
  };
  // one chunk: stage its A blocks, barrier, prefetch the A blocks of chunk+1 and the rows of chunk+PD,
  // 4 groups x (TB + TBE) MFMAs
  auto do_chunk = [&](int chunk, auto slotc, auto fastc) __attribute__((always_inline)) {
    constexpr bool FAST = decltype(fastc)::value;     // FAST: chunk+PD < c1 and all rows of both chunks exist
    constexpr int slot = decltype(slotc)::value;
    double* st = stage[(chunk - c0) & 1];
#pragma unroll
    for (int j = 0; j < YJ; ++j)
      if (tid + 256 * j < YA) st[tid + 256 * j] = ys[j];
#pragma unroll
    for (int j = 0; j < EJ; ++j)
      if (tid + 256 * j < EA) st[YA + tid + 256 * j] = es[j];
    __syncthreads();
    if (FAST || chunk + 1 < c1) load_a(chunk + 1);
    const bool more = FAST || chunk + PD < c1;
    if (active) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) {
        const double xq = (double)xn[slot][0][ti];
        bool ok = isfinite(xq) && isfinite((double)xn[slot][1][ti]) && isfinite((double)xn[slot][2][ti]);
        bool inrow = true;
        if (!FAST) inrow = (int64_t)chunk * 16 + ti * 4 + g < N;
        if (more) load_x(chunk + PD, slotc, ti, fastc);
        const double xs = (ok && inrow) ? xq : 0.0;          // a select: NaN * 0 is NaN
        const double miss = (!ok && inrow) ? 1.0 : 0.0;
#pragma unroll
        for (int t = 0; t < TB; ++t) acc[t] = TEMX_MFMA4(st[(ti * TB + t) * 16 + yoff], xs, acc[t]);
#pragma unroll
        for (int t = 0; t < TBE; ++t) acce[t] = TEMX_MFMA4(st[YA + (ti * TBE + t) * 16 + yoff], miss, acce[t]);
      }
    }
  };
  // PD consecutive chunks, ring slot = position in the unrolled group
  auto do_group = [&](int chunk, auto fastc) __attribute__((always_inline)) {
    do_chunk(chunk, std::integral_constant<int, 0>{}, fastc);
    if (PD > 1 && (decltype(fastc)::value || chunk + 1 < c1))
      do_chunk(chunk + 1, std::integral_constant<int, (PD > 1 ? 1 : 0)>{}, fastc);
    if (PD > 2 && (decltype(fastc)::value || chunk + 2 < c1))
      do_chunk(chunk + 2, std::integral_constant<int, (PD > 2 ? 2 : 0)>{}, fastc);
  };

  if (c0 < c1) {
    load_a(c0);
    if (active) {
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) load_x(c0, std::integral_constant<int, 0>{}, ti, std::false_type{});
      if (PD > 1 && c0 + 1 < c1) {
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
          load_x(c0 + 1, std::integral_constant<int, (PD > 1 ? 1 : 0)>{}, ti, std::false_type{});
      }
      if (PD > 2 && c0 + 2 < c1) {
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
          load_x(c0 + 2, std::integral_constant<int, (PD > 2 ? 2 : 0)>{}, ti, std::false_type{});
      }
    }
  }
  // chunks c with c + 2*PD - 1 < min(c1, nfull) run whole groups on the clamp-free path
  const int cfast = (c1 < nfull ? c1 : nfull) - (2 * PD - 1);
  int chunk = c0;
  for (; chunk < cfast; chunk += PD) do_group(chunk, std::true_type{});
  for (; chunk < c1; chunk += PD) do_group(chunk, std::false_type{});

  if (dvalid) {
    const int64_t R = (int64_t)K + NE;
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      const int l = t * 4 + g;
      if (l < K) partial[((int64_t)split * R + l) * D + d] = acc[t];
    }
#pragma unroll
    for (int t = 0; t < TBE; ++t) {
      const int n = t * 4 + g;
      if (n < NE) partial[((int64_t)split * R + K + n) * D + d] = acce[t];
    }
  }
}

// The three native tracer fields (tem_diagnostics.py:537, 563-567): qp, qpvp, qpwapp, each [N][D] or NULL.
// C: [3][K4][D] masked coefficients of (q, v, omega), Ccov: [K4][D] coverage coefficients of the tracer's mask.
// NaN where any of q, v, omega is not finite or the tracer's native coverage is below thr.  No scratch.
struct TracerEddyOut {
  double* p[3];
};

template <typename T>
__global__ void __launch_bounds__(256)
miss_tracer_native_kernel(FieldPtrs<3> fp, int64_t N, int64_t D, int K, int K4, const double* __restrict__ yblk,
                          int gstride, const double* __restrict__ C, const double* __restrict__ Ccov, double thr,
                          TracerEddyOut eo) {
  const int64_t total = N * D;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / D, d = idx - i * D;
    double rec[3] = {0.0, 0.0, 0.0}, cv = 0.0;
    for (int l = 0; l < K; ++l) {
      const double q = miss_q(yblk, gstride, i, l);
#pragma unroll
      for (int f = 0; f < 3; ++f) rec[f] += q * C[((int64_t)f * K4 + l) * D + d];
      cv += q * Ccov[(int64_t)l * D + d];
    }
    double x[3];
    bool ok = !(thr > 0.0 && !(cv >= thr));
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      x[f] = (double)reinterpret_cast<const T*>(fp.p[f])[idx];
      ok = ok && isfinite(x[f]);
    }
    const double qnan = __builtin_nan("");
    double e[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) e[f] = ok ? x[f] - rec[f] : qnan;
    if (eo.p[0]) eo.p[0][idx] = e[0];
    if (eo.p[1]) eo.p[1][idx] = e[0] * e[1];
    if (eo.p[2]) eo.p[2][idx] = e[0] * e[2];
  }
}

}  // namespace temx
