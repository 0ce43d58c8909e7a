// mgclim_shapes.hpp -- host: how a launch of the masked grouped time sum (kernels_mgclim.hpp,
// ../include/temx_mgclim.h) is cut.  Pure functions of sizes; no HIP.
//
// A workgroup holds `nfs` fields together: 1 in own-mask mode (the fields along the grid's y), nf under a common mask
// (nclim_shapes.hpp).  The order of the additions of a (row, group) is pinned to temxg_time_sum_groups, whose rows are
// cut by (nt, element size) alone (clim_shapes.hpp), so the form changes where that kernel's does:
//   staged    nt < clim_switch_nt(esz).  The nfs images of a workgroup's rows share NCLIM_LDS_BYTES as nclim_shape
//             splits them: `rpb` rows per image, a row every `stride` elements, stride odd.  Where nclim_shape would no
//             longer stage (fewer than NCLIM_MIN_ROWS rows fit), the rows that do fit are staged all the same, at least
//             two: a wave per row would add in another order.  A unit of work is (group present, row); unit u of a
//             workgroup with nr rows is (u / nr, u % nr), lane u % 256 takes it in round u / 256.
//   long row  a wave per row, the nfs values of a time in registers.  With at most 4 groups present (gclim_bound) the
//             accumulators are registers, NCLIM_LONG_ROWS rows per workgroup.  With more they live in a wave-private
//             LDS image [slot][output][64 lanes], one slot per group present and nfs + 2 outputs (the sums, the weights,
//             the count), so np * (nfs + 2) * 512 bytes: a workgroup takes as many waves (1 to 4) as fit
//             MGCLIM_LONG_LDS_BYTES, and where not even one does, the wave takes the groups present in batches of
//             mgclim_batch(nfs) slots, one walk of the row per batch.
#ifndef TEMX_MGCLIM_SHAPES_HPP
#define TEMX_MGCLIM_SHAPES_HPP
#include <cstddef>
#include <cstdint>

#include "gclim_tables.hpp"
#include "nclim_shapes.hpp"

namespace temx {

constexpr int MGCLIM_NFMAX = NCLIM_NFMAX;
constexpr int MGCLIM_NGMAX = GCLIM_NGMAX;
constexpr int MGCLIM_THREADS = NCLIM_THREADS;
constexpr int MGCLIM_STAGED_NT = 512;              // staged rows are shorter than this: the entries of the table's LDS copy
constexpr int MGCLIM_LONG_LDS_BYTES = 64 * 1024;   // LDS form of the long rows: the images of a workgroup's waves

// fields of one workgroup, and the instantiation (NFT) that holds them
inline int mgclim_nfs(int nf, bool common) { return common ? nf : 1; }
inline int mgclim_nft(int nf, bool common) { return !common ? 1 : nf <= 4 ? 4 : MGCLIM_NFMAX; }

// the smallest nt whose rows take a long-row form: that of the grouped sum, whatever nfs
inline int64_t mgclim_switch_nt(size_t esz) { return clim_switch_nt(esz); }

// bytes of one slot of a wave's LDS image, and the slots of one pass
inline int mgclim_slot_bytes(int nfs) { return (nfs + 2) * 64 * 8; }
inline int mgclim_batch(int nfs) { return MGCLIM_LONG_LDS_BYTES / mgclim_slot_bytes(nfs); }

// the (group present, row) of unit u in a staged workgroup of nr rows
inline void mgclim_unit(int u, int nr, int* q, int* r) { *q = u / nr, *r = u - (u / nr) * nr; }

struct MgclimShape {
  int staged;        // 1 staged kernel, 0 a long-row form
  int rpb;           // staged: rows per workgroup (of every image)
  int stride;        // staged: LDS elements per row, odd, >= nt
  int bound;         // long rows: gclim_bound(np); staged: 0
  int batch;         // LDS form: slots of one pass (<= mgclim_batch(nfs)); else 0
  int npass;         // LDS form: passes over the row, ceil(np / batch); else 1
  int rpw;           // rows per workgroup
  int64_t nblk;      // workgroups along x
  size_t lds_bytes;  // staged: the nfs images (<= NCLIM_LDS_BYTES); LDS form: rpw images (<= MGCLIM_LONG_LDS_BYTES)
};

inline MgclimShape mgclim_shape(int64_t rows, int64_t nt, size_t esz, int nfs, int np) {
  MgclimShape s{};
  s.npass = 1;
  if (clim_shape(rows, nt, esz).staged) {   // nt < mgclim_switch_nt(esz)
    const NclimShape n = nclim_shape(rows, nt, esz, nfs);
    const int64_t fit = nclim_fit(nt, esz, nfs);   // >= 2 here: 16 rows of one image fit, and nfs <= 8
    s.staged = 1;
    s.rpb = n.staged ? n.rpb : (int)fit;
    s.stride = (int)(nt | 1);
    s.rpw = s.rpb;
    s.lds_bytes = (size_t)nfs * (size_t)s.rpb * (size_t)s.stride * esz;
  } else {
    s.bound = gclim_bound(np);
    if (s.bound == GCLIM_NGMAX) {
      const int cap = mgclim_batch(nfs);
      s.batch = np < cap ? np : cap;
      s.npass = (np + s.batch - 1) / s.batch;
      const int fit = MGCLIM_LONG_LDS_BYTES / (s.batch * mgclim_slot_bytes(nfs));
      s.rpw = fit < 1 ? 1 : fit < NCLIM_LONG_ROWS ? fit : NCLIM_LONG_ROWS;
      s.lds_bytes = (size_t)s.rpw * (size_t)s.batch * (size_t)mgclim_slot_bytes(nfs);
    } else {
      s.rpw = NCLIM_LONG_ROWS;
    }
  }
  s.nblk = s.rpw > 0 ? (rows + s.rpw - 1) / s.rpw : 0;
  return s;
}

}  // namespace temx

#endif
