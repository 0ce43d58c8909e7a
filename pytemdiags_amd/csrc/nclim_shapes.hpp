// nclim_shapes.hpp -- host: how a launch of the time sum over valid times (kernels_nclim.hpp, include/temx_nclim.h) is
// cut.  Pure functions of sizes; no HIP.
//
// A field is R = ncol * nlev rows of nt elements, back to back.  A workgroup stages `nfs` fields together: 1 in
// own-mask mode (a field per workgroup, the fields along the grid's y), nf in common-mask mode (the workgroup that owns
// a set of rows holds those rows of all nf fields before it adds).  Two kernels, as in clim_shapes.hpp:
//   staged    a workgroup owns `rpb` consecutive rows: it loads their contiguous span of each of its nfs fields into an
//             LDS image of its own (`rpb * stride` elements, a row every `stride` elements, stride odd), then `g` lanes
//             per row sum it.  The NCLIM_LDS_BYTES of a workgroup are split evenly between the nfs images; rpb, stride
//             and g depend on (nt, element size, nfs) only, so the order of the additions of a row does too.
//   long row  a wave per row, NCLIM_LONG_ROWS rows per workgroup, the nfs fields of a time in registers; taken where
//             fewer than NCLIM_MIN_ROWS rows fit the LDS budget.  nclim_switch_nt(esz, nfs) is the first nt that takes it.
#ifndef TEMX_NCLIM_SHAPES_HPP
#define TEMX_NCLIM_SHAPES_HPP
#include <cstddef>
#include <cstdint>

namespace temx {

constexpr int NCLIM_NFMAX = 8;
constexpr int NCLIM_THREADS = 256;
constexpr int NCLIM_LDS_BYTES = 32 * 1024;   // all staged images of a workgroup: five workgroups share the 160 KiB of a CU's LDS
constexpr int NCLIM_MIN_ROWS = 16;           // fewer rows per workgroup than this: the long-row kernel
constexpr int NCLIM_LONG_ROWS = NCLIM_THREADS / 64;

struct NclimShape {
  int staged;      // 1 staged kernel, 0 long-row kernel
  int rpb;         // rows per workgroup
  int stride;      // staged: LDS elements per row, odd, >= nt
  int g;           // staged: lanes per row, a power of two, rpb * g <= NCLIM_THREADS, g <= 64
  int64_t nblk;    // workgroups along x: ceil(R / rpb)
};

// rows a workgroup can stage: esz bytes per element (8 or 4; the LDS images keep the source's dtype), nfs images
inline int64_t nclim_fit(int64_t nt, size_t esz, int nfs) {
  const int64_t budget = (int64_t)(NCLIM_LDS_BYTES / esz) / nfs;   // elements of one image
  const int64_t stride = nt | 1;
  return stride <= budget ? budget / stride : 0;
}

inline NclimShape nclim_shape(int64_t rows, int64_t nt, size_t esz, int nfs) {
  NclimShape s{};
  const int64_t fit = nclim_fit(nt, esz, nfs);
  if (fit >= NCLIM_MIN_ROWS) {
    s.staged = 1;
    s.rpb = (int)(fit < NCLIM_THREADS ? fit : NCLIM_THREADS);
    s.stride = (int)(nt | 1);
    s.g = 1;
    while (s.g < 64 && s.rpb * (s.g * 2) <= NCLIM_THREADS) s.g *= 2;
  } else {
    s.staged = 0;
    s.rpb = NCLIM_LONG_ROWS;
    s.stride = 0;
    s.g = 64;
  }
  s.nblk = (rows + s.rpb - 1) / s.rpb;
  return s;
}

// the smallest nt whose rows take the long-row kernel
inline int64_t nclim_switch_nt(size_t esz, int nfs) {
  int64_t nt = 1;
  while (nclim_fit(nt, esz, nfs) >= NCLIM_MIN_ROWS) ++nt;
  return nt;
}

}  // namespace temx

#endif
