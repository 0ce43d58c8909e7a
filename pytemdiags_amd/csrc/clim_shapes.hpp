// clim_shapes.hpp -- host: how a launch of the time sum (kernels_clim.hpp, include/temx_clim.h) is cut.
// Pure functions of sizes; no HIP.
//
// A field is R = ncol * nlev rows of nt elements, back to back.  Two kernels:
//   staged    a workgroup owns `rpb` consecutive rows: it loads their contiguous span into LDS (a row every `stride`
//             elements, stride odd), then `g` lanes per row sum it.  rpb, stride and g depend on (nt, element size) only,
//             so the order of the additions of a row does too.
//   long row  a wave per row, CLIM_LONG_ROWS rows per workgroup; taken where fewer than CLIM_MIN_ROWS rows fit the LDS
//             budget.  clim_switch_nt(esz) is the first nt that takes it.
#ifndef TEMX_CLIM_SHAPES_HPP
#define TEMX_CLIM_SHAPES_HPP
#include <cstddef>
#include <cstdint>

namespace temx {

constexpr int CLIM_NFMAX = 8;
constexpr int CLIM_THREADS = 256;
constexpr int CLIM_LDS_BYTES = 32 * 1024;   // staged image of a workgroup: five workgroups share the 160 KiB of a CU's LDS
constexpr int CLIM_MIN_ROWS = 16;           // fewer rows per workgroup than this: the long-row kernel
constexpr int CLIM_LONG_ROWS = CLIM_THREADS / 64;

struct ClimShape {
  int staged;      // 1 staged kernel, 0 long-row kernel
  int rpb;         // rows per workgroup
  int stride;      // staged: LDS elements per row, odd, >= nt
  int g;           // staged: lanes per row, a power of two, rpb * g <= CLIM_THREADS, g <= 64
  int64_t nblk;    // workgroups of one field: ceil(R / rpb)
};

// esz: bytes of a source element (8 or 4); the LDS image keeps the source's dtype
inline ClimShape clim_shape(int64_t rows, int64_t nt, size_t esz) {
  ClimShape s{};
  const int64_t budget = (int64_t)(CLIM_LDS_BYTES / esz);          // elements
  const int64_t stride = nt | 1;
  const int64_t fit = stride <= budget ? budget / stride : 0;
  if (fit >= CLIM_MIN_ROWS) {
    s.staged = 1;
    s.rpb = (int)(fit < CLIM_THREADS ? fit : CLIM_THREADS);
    s.stride = (int)stride;
    s.g = 1;
    while (s.g < 64 && s.rpb * (s.g * 2) <= CLIM_THREADS) s.g *= 2;
  } else {
    s.staged = 0;
    s.rpb = CLIM_LONG_ROWS;
    s.stride = 0;
    s.g = 64;
  }
  s.nblk = (rows + s.rpb - 1) / s.rpb;
  return s;
}

// the smallest nt whose rows take the long-row kernel
inline int64_t clim_switch_nt(size_t esz) {
  const int64_t budget = (int64_t)(CLIM_LDS_BYTES / esz);
  int64_t nt = 1;
  while (((nt | 1) <= budget ? budget / (nt | 1) : 0) >= CLIM_MIN_ROWS) ++nt;
  return nt;
}

}  // namespace temx

#endif
