// kernels_tfilt.hpp -- a finite-impulse-response filter along the time axis of fields in the engine's layout
// (../include/temx_tfilt.h, temxf_filter_time).
//
// NF sources [ncol][nlev][nt] (time fastest, fp64 or fp32 each) -> NB x NF destinations [ncol][nlev][nto], nto = nt - nw + 1:
//   dst[b][f][r][t] = round( sum_k w[b][k] (double) src[f][r][t + k] ),   acc = fma(w[b][k], x, acc), k ascending from +0.0.
// A field is rows = ncol * nlev rows of nt elements back to back.  tfilt_shapes.hpp cuts the launch: a workgroup owns rpb
// consecutive rows by a tile of TT output times.
//   load side     the rpb x (tw + nw - 1) source span of the tile (tw = TT, less in the last tile) goes to LDS in the
//                 source dtype, a row every `stride` elements, stride odd.  A wave takes every fourth row, its lanes run
//                 along time (element loads, a wave instruction covers 64 consecutive elements), TFILT_BATCH rows in
//                 flight per lane before the first goes to LDS.
//   filter side   lane l works on row l % rpb, so that the lanes of a wave read one time of neighbouring rows: with an odd
//                 stride a ds_read_b64 (fp64) or ds_read_b32 (fp32) of 32 such lanes is free of bank conflicts whenever
//                 rpb >= 32.  The 256 / rpb lanes of a row take its runs of R = 8 consecutive outputs in turn.  A run holds
//                 a window of R elements in registers, element e in slot e % R: step k multiplies the window by w[b][k] for
//                 every band b and output j, then replaces element k by element k + R.  The k loop is unrolled by R, so the
//                 slots are static registers; every staged element is read from LDS once per run it belongs to,
//                 (R + nw - 1) / R reads per output instead of nw.  The weights are uniform over the wave: they come from
//                 the device table through scalar loads (w is const, restrict and indexed by k alone).
//   All NB bands of an output come from the same window: the record is read once and written NB times.
// The bits of an output are those of its chain of nw fused multiply-adds: they do not depend on the cut, the lane or the
// position of the row.  Elements of LDS beyond the span are read only into outputs that are not stored.  Nothing is
// written outside dst[b][f][0 .. rows * nto): each output is stored once, by one lane.  All global offsets are int64_t.
#pragma once
#include "tfilt_shapes.hpp"
#include <hip/hip_runtime.h>

#include <cstdint>

namespace temx {

constexpr int TFILT_BATCH = 4;   // rows in flight per lane on the load side

struct TfiltPtrs {
  const void* src[TFILT_NF_MAX];
  void* dst[TFILT_NB_MAX][TFILT_NF_MAX];
};

// grid (sh.grid, nf): the nf sources of one launch share the element type T; D is the destination's
template <typename T, typename D, int NB>
__global__ void __launch_bounds__(TFILT_THREADS)
tfilt_kernel(TfiltPtrs fp, const double* __restrict__ w, int64_t rows, int64_t nt, int nw, TfiltShape sh) {
  constexpr int R = TFILT_R;
  __shared__ __attribute__((aligned(16))) unsigned char tfilt_lds[TFILT_LDS_BYTES];
  T* s = reinterpret_cast<T*>(tfilt_lds);
  const int f = blockIdx.y;
  const T* __restrict__ src = nullptr;
  D* __restrict__ dst[NB];
#pragma unroll
  for (int q = 0; q < TFILT_NF_MAX; ++q)
    if (q == f) {
      src = reinterpret_cast<const T*>(fp.src[q]);
#pragma unroll
      for (int b = 0; b < NB; ++b) dst[b] = reinterpret_cast<D*>(fp.dst[b][q]);
    }
  const int64_t nto = nt - nw + 1;
  const int64_t rb = (int64_t)blockIdx.x / sh.ntile;
  const int tile = (int)((int64_t)blockIdx.x - rb * sh.ntile);
  const int64_t r0 = rb * sh.rpb;
  if (r0 >= rows) return;   // (uniform; the host launches exactly ntile * ceil(rows / rpb) workgroups per field)
  const int nr = (int)(rows - r0 < sh.rpb ? rows - r0 : sh.rpb);       // valid rows of this workgroup
  const int64_t t0 = (int64_t)tile * sh.TT;
  const int tw = (int)(nto - t0 < sh.TT ? nto - t0 : sh.TT);          // outputs per row of this tile
  const int span = tw + nw - 1;                                       // source elements per row: t0 + span <= nt
  const int stride = sh.stride;
  const int tid = threadIdx.x;

  // ---- load side: element e of row r -> s[r * stride + e] ----
  {
    const int lane = tid & 63, wv = tid >> 6;
    const T* p = src + r0 * nt + t0;
    for (int rbase = wv; rbase < nr; rbase += 4 * TFILT_BATCH)
      for (int e = lane; e < span; e += 64) {
        T v[TFILT_BATCH];
#pragma unroll
        for (int q = 0; q < TFILT_BATCH; ++q) {
          const int r = rbase + 4 * q;
          if (r < nr) v[q] = p[(int64_t)r * nt + e];
        }
#pragma unroll
        for (int q = 0; q < TFILT_BATCH; ++q) {
          const int r = rbase + 4 * q;
          if (r < nr) s[r * stride + e] = v[q];
        }
      }
  }
  __syncthreads();

  // ---- filter side ----
  const int r = tid & (sh.rpb - 1);
  if (r >= nr) return;
  const int rl = tid / sh.rpb, step = (TFILT_THREADS / sh.rpb) * R;
  for (int j0 = rl * R; j0 < tw; j0 += step) {
    const T* p = s + r * stride + j0;      // the run reads p[0 .. R + nw - 1): j0 + R <= TT, inside the row's stride
    double x[R], acc[NB][R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      x[j] = (double)p[j];
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[b][j] = 0.0;
    }
    int k0 = 0;
    for (; k0 + R <= nw; k0 += R) {        // (nw is odd: k + 1 < nw throughout, every refill is inside the run)
#pragma unroll
      for (int kk = 0; kk < R; ++kk) {
        const int k = k0 + kk;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const double wk = w[b * nw + k];
#pragma unroll
          for (int j = 0; j < R; ++j) acc[b][j] = __builtin_fma(wk, x[(j + kk) % R], acc[b][j]);
        }
        x[kk] = (double)p[k + R];
      }
    }
#pragma unroll
    for (int kk = 0; kk < R; ++kk) {
      const int k = k0 + kk;
      if (k < nw) {                        // (uniform)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          const double wk = w[b * nw + k];
#pragma unroll
          for (int j = 0; j < R; ++j) acc[b][j] = __builtin_fma(wk, x[(j + kk) % R], acc[b][j]);
        }
        if (k + 1 < nw) x[kk] = (double)p[k + R];
      }
    }
    const int64_t o = (r0 + r) * nto + t0 + j0;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int j = 0; j < R; ++j)
        if (j0 + j < tw) dst[b][o + j] = (D)acc[b][j];
  }
}

}  // namespace temx
