// tfilt_shapes.hpp -- host: the argument rules of temxf_filter_time (kernels_tfilt.hpp, ../include/temx_tfilt.h) and how
// a launch of it is cut.  Pure functions of sizes and addresses; no HIP.  tests/host/tfilt_shapes_main.cpp runs this
// header under the sanitizers.
//
// A field is rows = ncol * nlev rows of nt elements, back to back; a row gives nto = nt - nw + 1 outputs.  A workgroup of
// TFILT_THREADS lanes owns rpb consecutive rows (a power of two) by a tile of TT consecutive output times (a multiple of
// R): it stages the rpb x (TT + nw - 1) source span in LDS in the source dtype, a row every `stride` elements, stride
// odd.  Lane l works on row l % rpb: consecutive lanes read one time of neighbouring rows, which an odd stride puts into
// different banks.  The 256 / rpb lanes of a row take its runs of R consecutive outputs in turn.
//
// The cut.  rpb = 32 and a TT of whole rounds of its 8 lanes per row where that fits the LDS budget; more rows per
// workgroup where a row has fewer runs than lanes (short records), fewer where the halo leaves no room (fp64 with
// nw > 96: 16 rows, nw > 192: 8).  The bits of an output do not depend on the cut: every output is the same chain of nw
// fused multiply-adds whichever lane forms it.
#ifndef TEMX_TFILT_SHAPES_HPP
#define TEMX_TFILT_SHAPES_HPP
#include <cstddef>
#include <cstdint>

#include "field_args.hpp"

namespace temx {

constexpr int TFILT_NF_MAX = 8;
constexpr int TFILT_NB_MAX = 4;
constexpr int TFILT_NW_MAX = 255;
constexpr int TFILT_THREADS = 256;
constexpr int TFILT_R = 8;                    // consecutive outputs per lane and run: the width of the register window
constexpr int TFILT_LDS_BYTES = 40 * 1024;    // staged image of a workgroup: four workgroups share the 160 KiB of a CU's LDS
constexpr int64_t TFILT_GRID_MAX = (int64_t(1) << 32) / TFILT_THREADS;   // HIP takes fewer than 2^32 threads per grid dimension

struct TfiltShape {
  int rpb;        // rows per workgroup, a power of two <= TFILT_THREADS
  int TT;         // output times per tile, a multiple of TFILT_R
  int stride;     // LDS elements per row, odd, >= TT + nw - 1
  int R;          // TFILT_R
  int ntile;      // tiles along time: ceil(nto / TT)
  int64_t grid;   // workgroups of one field: ntile * ceil(rows / rpb); workgroup g is row block g / ntile, tile g % ntile
};

inline size_t tfilt_lds_bytes(const TfiltShape& s, size_t src_esz) { return (size_t)s.rpb * s.stride * src_esz; }

// rows, nt >= nw, nw odd in 1..TFILT_NW_MAX, src_esz 4 or 8 (tfilt_check_sizes has seen them).  nb and dst_esz do not move
// the cut: the bands of an output share its window and the outputs go from registers to memory.
inline TfiltShape tfilt_shape(int64_t rows, int64_t nt, int nw, int /*nb*/, size_t src_esz, size_t /*dst_esz*/) {
  TfiltShape s{};
  s.R = TFILT_R;
  const int64_t nto = nt - nw + 1;
  const int64_t budget = (int64_t)(TFILT_LDS_BYTES / src_esz);                  // elements
  const int64_t full = (nto + TFILT_R - 1) / TFILT_R * TFILT_R;                  // a whole row, in whole runs
  for (int rpb = TFILT_THREADS; rpb >= 1; rpb /= 2) {
    const int64_t unit = (int64_t)(TFILT_THREADS / rpb) * TFILT_R;               // outputs of one round of a row's lanes
    int64_t cap = (budget / rpb - 1 - (nw - 1)) / TFILT_R * TFILT_R;              // (TT + nw - 1) | 1 <= budget / rpb
    if (cap < TFILT_R) continue;
    int64_t TT;
    if (rpb > 32) {
      if (full > unit || full > cap) continue;       // many rows per workgroup only for rows of at most one round
      TT = full;
    } else {
      if (cap < unit && cap < full && rpb > 1) continue;
      TT = cap >= unit ? cap / unit * unit : cap;
      if (TT > full) TT = full;
    }
    s.rpb = rpb;
    s.TT = (int)TT;
    break;
  }
  s.stride = (int)((s.TT + nw - 1) | 1);
  s.ntile = (int)((nto + s.TT - 1) / s.TT);
  s.grid = (int64_t)s.ntile * ((rows + s.rpb - 1) / s.rpb);
  return s;
}

// the scalar rules of temxf_filter_time and temxf_filter_shape
inline Refusal tfilt_check_sizes(int64_t rows_or_ncol, int nlev, int64_t nt, int nw, int nb) {
  if (nb < 1 || nb > TFILT_NB_MAX) return refuse("nb must lie in 1..%d, got %d", TFILT_NB_MAX, nb);
  if (nw < 1 || nw > TFILT_NW_MAX) return refuse("nw must lie in 1..%d, got %d", TFILT_NW_MAX, nw);
  if (nw % 2 == 0) return refuse("nw must be odd (a centred filter), got %d", nw);
  if (Refusal r = check_sizes(rows_or_ncol, nlev, nt, "nt")) return r;
  if (nt < nw) return refuse("nt = %lld is shorter than the filter (nw = %d)", (long long)nt, nw);
  return {};
}

// every rule of temxf_filter_time, in the order the header lists them.  dst_host: [nb][nf] pointers.
inline Refusal tfilt_check_args(int nf, const void* const* src_host, const int* src_dtype_host, int nb, void* const* dst_host,
                                int dst_dtype, int64_t ncol, int nlev, int64_t nt, int nw, const double* weights, int flags) {
  if (Refusal r = check_nf(nf, TFILT_NF_MAX) | check_null(src_host, "src_host") | check_null(src_dtype_host, "src_dtype_host") |
                  check_null(dst_host, "dst_host") | check_null(weights, "weights") | check_dtype(dst_dtype, "dst_dtype") |
                  check_flags(flags, 0) | tfilt_check_sizes(ncol, nlev, nt, nw, nb))
    return r;
  const size_t rows = (size_t)ncol * nlev, dsz = dtype_size(dst_dtype);
  const size_t src_elems = rows * (size_t)nt, dst_bytes = rows * (size_t)(nt - nw + 1) * dsz, w_bytes = (size_t)nb * nw * sizeof(double);
  if ((uintptr_t)weights % sizeof(double)) return refuse("weights is not aligned to its element size");
  for (int f = 0; f < nf; ++f) {
    if (src_dtype_host[f] != TEMX_F64 && src_dtype_host[f] != TEMX_F32) return refuse("src_dtype %d must be TEMX_F64 or TEMX_F32", f);
    if (src_dtype_host[f] == TEMX_F64 && dst_dtype == TEMX_F32)
      return refuse("src_dtype %d is TEMX_F64 but dst_dtype is TEMX_F32: this call does not narrow", f);
    if (!src_host[f]) return refuse("src %d is null", f);
    if ((uintptr_t)src_host[f] % dtype_size(src_dtype_host[f])) return refuse("src %d is not aligned to its element size", f);
  }
  const int nd = nb * nf;
  for (int i = 0; i < nd; ++i) {
    if (!dst_host[i]) return refuse("dst %d (band %d, field %d) is null", i, i / nf, i % nf);
    if ((uintptr_t)dst_host[i] % dsz) return refuse("dst %d (band %d, field %d) is not aligned to its element size", i, i / nf, i % nf);
  }
  for (int i = 0; i < nd; ++i) {
    if (extents_overlap(dst_host[i], dst_bytes, weights, w_bytes)) return refuse("dst %d overlaps weights", i);
    for (int g = 0; g < nf; ++g)
      if (extents_overlap(dst_host[i], dst_bytes, src_host[g], src_elems * dtype_size(src_dtype_host[g])))
        return refuse("dst %d overlaps src %d", i, g);
    for (int g = 0; g < i; ++g)
      if (extents_overlap(dst_host[i], dst_bytes, dst_host[g], dst_bytes)) return refuse("dst %d overlaps dst %d", i, g);
  }
  return {};
}

}  // namespace temx

#endif
