// launch_shapes.hpp -- host: how a launch is cut (choose_split) and the LDS shapes of the vertical interpolation
// and of the re-layout.  Pure functions of sizes; no HIP.
#ifndef TEMX_LAUNCH_SHAPES_HPP
#define TEMX_LAUNCH_SHAPES_HPP
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "shared_defs.hpp"

namespace temx {

struct Split {
  int ndt = 0, nsplit = 0, grid = 0, dpw = 4;   // dpw: d-tiles per workgroup
};

// How to cut (d-tiles x chunk range) into wave-sized work so that `slots` workgroup slots
// (CUs x resident workgroups) are evenly filled.  Smaller nsplit is preferred on near-ties
// (fewer partial slabs to write and re-read).
inline Split choose_split(int64_t D, int64_t nchunk, int slots, int dpw = 4, int minchunk = 4) {
  Split s;
  s.dpw = dpw;
  s.ndt = (int)((D + 15) / 16);
  const int ndq = (s.ndt + dpw - 1) / dpw;    // a workgroup owns dpw consecutive d-tiles
  int64_t maxsplit = std::max<int64_t>(1, nchunk / minchunk);
  maxsplit = std::min<int64_t>(maxsplit, std::max<int64_t>(1, (int64_t)4 * slots / ndq + 1));
  maxsplit = std::min<int64_t>(maxsplit, 4096);
  double best = -1.0;
  int bestn = 1;
  for (int n = 1; n <= maxsplit; ++n) {
    const int64_t nwg = (int64_t)ndq * n;
    const int64_t rounds = (nwg + slots - 1) / slots;
    const double eff = (double)nwg / (double)(rounds * slots);
    if (eff > best * 1.02) {
      best = eff;
      bestn = n;
    }
  }
  s.nsplit = bestn;
  const int64_t nwg = (int64_t)ndq * s.nsplit;
  s.grid = (int)(((nwg + 7) / 8) * 8);
  return s;
}

// The slab-staged map: how many columns a workgroup takes and how their walks are cut, from an LDS budget of 48 KiB
// (three workgroups per CU: one loads while another walks).  false: one column does not fit (long rows).
inline bool vert_slab_shape(int nf, int nlev, int64_t nt, int nplev, size_t tsz, size_t psz, VertSlab* sh, size_t* lds) {
  if (nt > VERT_THREADS / 4) return false;
  const int colsz = nlev * (int)nt, ocolsz = nplev * (int)nt;
  sh->in_stride = colsz | 1;
  sh->out_stride = ocolsz | 1;
  const size_t percol = (size_t)nf * (sh->in_stride + sh->out_stride) * tsz + (size_t)sh->in_stride * psz;
  const size_t budget = 48 * 1024 - VERT_THREADS * sizeof(int) - (2 * nf + 1) * 16;
  int cw = (int)std::min<size_t>(budget / percol, (size_t)(VERT_THREADS / nt));
  if (cw < 1) return false;
  sh->cw = cw;
  const int pairs = cw * (int)nt, brackets = nlev - 1, most = VERT_THREADS / pairs;
  sh->seg = std::max(4, (brackets + most - 1) / most);
  sh->nseg = (brackets + sh->seg - 1) / sh->seg;
  auto r16 = [](size_t b) { return (int)((b + 15) & ~(size_t)15); };
  sh->in_img = r16((size_t)cw * sh->in_stride * tsz);
  sh->out_img = r16((size_t)cw * sh->out_stride * tsz);
  sh->p_img = r16((size_t)cw * sh->in_stride * psz);
  *lds = VERT_THREADS * sizeof(int) + sh->p_img + (size_t)nf * (sh->in_img + sh->out_img);
  return true;
}

// ---- re-layout: tile of a launch (kernels_layout.hpp) -----------------------------------------------------------
// rmax rows of 64 columns fill the 32 KiB tile.  A window of ntb <= rmax times moves whole, with as many levels per
// tile as fit (the run a column writes is kl * ntb elements); up to 2 rmax it still moves whole, over 32 columns;
// a longer one is cut into chunks of rmax times, one level per tile.
inline LayoutTile layout_tile(int64_t ncol, int nlev, int64_t ntb, size_t dsz) {
  LayoutTile tl{};
  const int rmax = (int)(32 * 1024 / (64 * dsz));
  tl.tc_shift = 6;
  if (ntb <= rmax) {
    tl.tt = (int)ntb;
    tl.kl = std::max(1, std::min(nlev, rmax / (int)ntb));
  } else if (ntb <= 2 * rmax) {
    tl.tc_shift = 5;
    tl.tt = (int)ntb;
    tl.kl = 1;
  } else {
    tl.tt = rmax;
    tl.kl = 1;
  }
  tl.stride = (tl.kl * tl.tt) | 1;
  tl.nct = (int)((ncol + (1 << tl.tc_shift) - 1) >> tl.tc_shift);
  tl.nlt = (nlev + tl.kl - 1) / tl.kl;
  tl.ntt = (int)((ntb + tl.tt - 1) / tl.tt);
  return tl;
}

// ---- fused ingestion: tile of a launch (kernels_ingest.hpp) -----------------------------------------------------
// dsz: bytes of a destination element; ssz: bytes of the narrowest source element.
//   TT   times per tile: 128 bytes of destination (what the lanes of one column write per target level), or the whole
//        window when it is shorter; halved until two level slots of all nf fields fit INGEST_LDS_BYTES.
//   TC   columns per tile: 128 bytes of the narrowest source per row on the read side (16 fp64, 32 fp32), more when
//        TT is short, so that the tile still has a (column, time) pair for every lane.
//   KW   brackets per level window: as many level slots as the budget holds, less one.
// false: no tile fits the budget (cannot happen for nf <= 8: TC = 256, TT = 1 takes 2 KiB per field and slot).
inline bool ingest_tile(int64_t ncol, int nlev, int64_t ntb, int nf, size_t dsz, size_t ssz, IngestTile* tl, size_t* lds) {
  if (ncol < 1 || nlev < 2 || ntb < 1 || nf < 1) return false;
  int tt = (int)std::min<int64_t>(ntb, (int64_t)(128 / dsz));
  for (;; tt = (tt + 1) / 2) {
    int shift = ssz >= 8 ? 4 : 5;
    while ((2 << shift) * tt <= INGEST_THREADS) ++shift;
    const int stride = tt | 1;
    const size_t img = ((size_t)1 << shift) * stride;
    const size_t slot = (size_t)nf * img * dsz, psb = img * sizeof(double);
    const size_t nslot = psb < (size_t)INGEST_LDS_BYTES ? ((size_t)INGEST_LDS_BYTES - psb) / slot : 0;
    if (nslot >= 2) {
      tl->tc_shift = shift;
      tl->tt = tt;
      tl->kw = (int)std::min<size_t>(nslot - 1, (size_t)nlev - 1);
      tl->stride = stride;
      tl->ppl = ((1 << shift) * tt + INGEST_THREADS - 1) / INGEST_THREADS;
      tl->nct = (int)((ncol + (1 << shift) - 1) >> shift);
      tl->ntt = (int)((ntb + tt - 1) / tt);
      tl->nwin = (nlev - 1 + tl->kw - 1) / tl->kw;
      *lds = psb + (size_t)(tl->kw + 1) * slot;
      return true;
    }
    if (tt == 1) return false;
  }
}

}  // namespace temx

#endif
