// class_tables.hpp -- host: the tables that tell the latitude-class sweeps (kernels_cls.hpp, kernels_op.hpp,
// kernels_op2.hpp) and the mirror-paired sweeps (kernels_sym.hpp) which rows to read: the mirror pairs, the row table
// crow with its flag bits and padding, its split per side (side_tables.hpp), the work cuts and the subsample of
// class-groups of the single sweep's pre-pass.  Arrays and sizes in, std::vectors out; no HIP, no plan, no environment.
#ifndef TEMX_CLASS_TABLES_HPP
#define TEMX_CLASS_TABLES_HPP
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "shared_defs.hpp"
#include "side_tables.hpp"

namespace temx {

// ---- mirror pairing of an equatorially symmetric grid (kernels_sym.hpp) -------------------------------------------
// Every column with lat > tol must have a partner with the opposite latitude (any longitude);
// |lat| <= tol are equator columns (pairs without a southern partner).  Returns false if the grid is
// not symmetric.  Pairs are ordered by their northern row so one operand still streams.
inline bool find_mirror_pairs(const double* lat, int64_t N, std::vector<int>& rowN, std::vector<int>& rowS, double tol) {
  if (N >= ((int64_t)1 << 31)) return false;
  // Two columns pair up when their latitudes are opposite to within `tol` degrees; the pair is then
  // treated as sitting exactly at +-(northern latitude), which perturbs the operator by
  // O(L^2 tol).  The caller's default keeps that below the fp64 parity tolerance.
  std::vector<int> north, south, eq;
  for (int64_t i = 0; i < N; ++i) {
    if (!(std::fabs(lat[i]) <= 90.0 + 1e-9)) return false;
    if (lat[i] > tol) north.push_back((int)i);
    else if (lat[i] < -tol) south.push_back((int)i);
    else eq.push_back((int)i);
  }
  if (north.size() != south.size()) return false;
  std::stable_sort(north.begin(), north.end(), [&](int a, int b) { return lat[a] < lat[b]; });
  std::stable_sort(south.begin(), south.end(), [&](int a, int b) { return -lat[a] < -lat[b]; });
  std::vector<std::pair<int, int>> pairs;
  pairs.reserve(north.size() + eq.size());
  for (size_t k = 0; k < north.size(); ++k) {
    if (std::fabs(lat[north[k]] + lat[south[k]]) > tol) return false;
    pairs.emplace_back(north[k], south[k]);
  }
  for (int e : eq) pairs.emplace_back(e, -1);
  std::sort(pairs.begin(), pairs.end());
  rowN.resize(pairs.size());
  rowS.resize(pairs.size());
  for (size_t k = 0; k < pairs.size(); ++k) {
    rowN[k] = pairs[k].first;
    rowS[k] = pairs[k].second;
  }
  return true;
}

// ---- latitude classes (kernels_cls.hpp) ---------------------------------------------------------------------------
// build_classes returns false when the grid has too few columns per class
// for the class sweeps to pay (the paired or generic sweeps are used instead).
struct ClassTables {
  std::vector<int> crow;        // [nbatch + CLS_PADB][4][CLS_MB]
  std::vector<double> xc;       // [4 * (ngroups + 1)] cos(colat) of the class latitude
  std::vector<int> gbatch0;     // [ngroups + 1]
  std::vector<double> cnt;      // [ngroups][2 sides][4 classes] member counts
  int64_t ncls = 0, ngroups = 0, nbatch = 0;
  int64_t max_side = 0;         // members of the longest class side
};

// Longest class side of a plan for fp32 fields (TEMX_LAT_TOL_F32).  sweep_os2_kernel adds the members of a side into
// ONE fp32 accumulator in sequence: with terms of size <= A (the eddy amplitude) the partial sum after k members is
// <= k A and the k-th addition rounds by <= k A 2^-24, so the sum of n members is off by <= A 2^-24 n^2 / 2 and the
// side mean S~ / n (and likewise q~ / n in units of A^2) by <= n 2^-25 -- call it n 2^-24 with the rounding of the
// differences themselves.  The fp32 path is held to 2e-5 of the field maximum; a tenth of that, 2e-6, allows
// n <= 2e-6 x 2^24 = 33.  But the bound is in units of the eddy AMPLITUDE, and a flux mean is normalised by the
// flux: with waves in quadrature (u' ~ sin 4 lon, v' ~ cos 4 lon, the fields of the test suite) max |u'v' mean| is
// about A^2 / 10, and a part of a lat-lon row spans enough longitude for the whole wave to enter its sums.  Sides
// of 32 measured 1.6e-5 ... 2.5e-5 of max |u'v' mean| on rows of 352 and 360 columns, sides of 8 -- the side of a
// cubed sphere, whose members lie all around the globe -- 5e-6.  Hence parts of 8: n 2^-24 = 4.8e-7, forty times
// under 2e-5 in units of A^2 and four times under it in the unit the results are compared in; two whole batches.
// A side of up to TEMX_F32_SIDE_KEEP = 16 members is left whole: at the 1e-8 degrees of an fp32 plan five pairs of
// neighbouring latitudes of ne240 fall into one class of 16 + 16, and the class tables of the cubed spheres that are
// timed (ne30, ne120, ne240) stay as they were, bit for bit.
#ifndef TEMX_F32_SIDE_CAP
#define TEMX_F32_SIDE_CAP 8
#endif
#ifndef TEMX_F32_SIDE_KEEP
#define TEMX_F32_SIDE_KEEP 16
#endif

struct LatClass {
  double alat;               // |lat| of the class, degrees
  std::vector<int> n, s;     // northern (and equator) rows, southern rows, ascending
};

// Appends c to `out` cut into classes at the same latitude that take cap_n northern and cap_s southern members each,
// in member order.  (No part is empty: part k exists because k * cap < size on the side that needs the most parts.)
inline void cut_class(const LatClass& c, size_t cap_n, size_t cap_s, std::vector<LatClass>& out) {
  const size_t parts = std::max((c.n.size() + cap_n - 1) / cap_n, (c.s.size() + cap_s - 1) / cap_s);
  for (size_t k = 0; k < parts; ++k) {
    LatClass d;
    d.alat = c.alat;
    if (k * cap_n < c.n.size()) d.n.assign(c.n.begin() + k * cap_n, c.n.begin() + std::min((k + 1) * cap_n, c.n.size()));
    if (k * cap_s < c.s.size()) d.s.assign(c.s.begin() + k * cap_s, c.s.begin() + std::min((k + 1) * cap_s, c.s.size()));
    out.push_back(std::move(d));
  }
}

// tol: two columns share a class when their |lat| agree to within tol degrees.  side_cap / side_keep: the cut of an
// fp32 plan (above); 0 = none.
inline bool build_classes(const double* lat, int64_t N, ClassTables& ct, double tol, size_t side_cap = 0,
                          size_t side_keep = 0) {
  if (N >= ((int64_t)1 << 27) || N < 64) return false;     // row indices live in 27 bits of a table entry
  std::vector<int> order((size_t)N);
  for (int64_t i = 0; i < N; ++i) {
    if (!(std::fabs(lat[i]) <= 90.0 + 1e-9)) return false;
    order[(size_t)i] = (int)i;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return std::fabs(lat[a]) < std::fabs(lat[b]); });
  std::vector<LatClass> cls;
  for (size_t i = 0; i < order.size();) {
    LatClass c;
    c.alat = std::fabs(lat[order[i]]);
    size_t j = i;
    for (; j < order.size() && std::fabs(lat[order[j]]) - c.alat <= tol; ++j) {
      const int r = order[j];
      (lat[r] < -tol ? c.s : c.n).push_back(r);      // equator columns count as northern
    }
    // the class sits at the mean |lat| of its members (they agree to within tol): deviations of either
    // sign, half the size of those from the smallest member
    long double sum = 0.0L;
    for (size_t m = i; m < j; ++m) sum += (long double)std::fabs(lat[order[m]]) - (long double)c.alat;
    c.alat += (double)(sum / (long double)(j - i));
    std::sort(c.n.begin(), c.n.end());
    std::sort(c.s.begin(), c.s.end());
    cls.push_back(std::move(c));
    i = j;
  }
  if ((double)N < 3.0 * (double)cls.size()) return false;   // < 3 columns per class: not worth it
  constexpr int MB = CLS_MB;
  auto nb = [](size_t m) { return (int)((m + MB - 1) / MB); };
  // Outsized classes are cut into several classes at the same latitude.  Any subset of the columns of a
  // latitude is a class (the algebra of kernels_cls.hpp holds per class side), and a class-group is the unit of
  // work between two hand-overs of the shared-d-tile sweep and of the work cuts: the cubed sphere has ONE
  // class of 1440 equator columns (360 batches) among 48 000 of 8 + 8 (4 batches), and every workgroup that
  // met it ran 20 % longer -- all of them on one XCD (ne120 x 72 x 30, TEM + tracer sweep: 17.6 -> 14 ms).
  {
    std::map<std::pair<size_t, size_t>, size_t> hist;
    for (const LatClass& c : cls) ++hist[{c.n.size(), c.s.size()}];
    std::pair<size_t, size_t> typ{0, 0};
    size_t best = 0;
    for (const auto& kv : hist)
      if (kv.second > best) {
        best = kv.second;
        typ = kv.first;
      }
    const size_t cap_n = std::max<size_t>(typ.first, MB), cap_s = std::max<size_t>(typ.second, MB);
    const int typ_b = std::max(1, nb(typ.first) + nb(typ.second));
    std::vector<LatClass> out;
    out.reserve(cls.size());
    for (LatClass& c : cls) {
      if (nb(c.n.size()) + nb(c.s.size()) <= 4 * typ_b) {
        out.push_back(std::move(c));
        continue;
      }
      cut_class(c, cap_n, cap_s, out);
    }
    cls.swap(out);
  }
  // fp32 plans: a side longer than side_keep members is cut into parts of side_cap (TEMX_F32_SIDE_CAP above).  A
  // lat-lon, Gaussian or HEALPix-like grid has NLON members per side and NLON is the TYPICAL size there, so the cut
  // above leaves them whole.  Each part is a class of its own at the same latitude, with its own first member as the
  // origin of its sums.  Classes within side_keep -- every class of a cubed sphere from ne8 on, whose equator the cut
  // above already took to 8 + 8 -- are not touched, and the order of the others among them is kept: a table without
  // a long side comes out bit for bit as before.
  if (side_cap) {
    bool any = false;
    for (const LatClass& c : cls) any = any || c.n.size() > side_keep || c.s.size() > side_keep;
    if (any) {
      std::vector<LatClass> out;
      out.reserve(cls.size());
      for (LatClass& c : cls) {
        if (c.n.size() <= side_keep && c.s.size() <= side_keep) {
          out.push_back(std::move(c));
          continue;
        }
        cut_class(c, side_cap, side_cap, out);
      }
      cls.swap(out);
    }
  }
  for (const LatClass& c : cls) ct.max_side = std::max<int64_t>(ct.max_side, (int64_t)std::max(c.n.size(), c.s.size()));
  // equal member counts inside a class-group; then by first row (some streaming order)
  std::stable_sort(cls.begin(), cls.end(), [&](const LatClass& a, const LatClass& b) {
    const int an = nb(a.n.size()), as = nb(a.s.size()), bn = nb(b.n.size()), bs = nb(b.s.size());
    if (an != bn) return an > bn;
    if (as != bs) return as > bs;
    const int ar = a.n.empty() ? a.s[0] : a.n[0], br = b.n.empty() ? b.s[0] : b.n[0];
    return ar < br;
  });
  // The class-groups (4 consecutive classes) of the few small strata -- ne240: 361 groups of 4 + 4 members and 90 of
  // 8 + 0 behind 48 374 of 8 + 8 -- are spread evenly among the others: a work cut is a run of consecutive groups
  // balanced by batch count, and the end of a group costs about as much as two batches, so the workgroup that got
  // the tail of a size-sorted table ran 30 % longer than the rest (ne240 x 128 x 1: 1.9 instead of 1.5 ms;
  // profiles/r03_lab20_class_order_d128_f32.log).  Inside a stratum the order stays.  A last, partial group stays last.
  {
    const size_t ngr = (cls.size() + 3) / 4;
    std::vector<std::pair<int, int>> shape(ngr);
    std::map<std::pair<int, int>, size_t> count, seen;
    for (size_t gi = 0; gi < ngr; ++gi) {
      int bN = 0, bS = 0;
      for (size_t ci = gi * 4; ci < std::min(gi * 4 + 4, cls.size()); ++ci) {
        bN = std::max(bN, nb(cls[ci].n.size()));
        bS = std::max(bS, nb(cls[ci].s.size()));
      }
      shape[gi] = {bN, bS};
      ++count[shape[gi]];
    }
    std::vector<std::pair<double, size_t>> key(ngr);
    for (size_t gi = 0; gi < ngr; ++gi) {
      const size_t i = seen[shape[gi]]++;
      key[gi] = {((double)i + 0.5) / (double)count[shape[gi]], gi};
      if (gi + 1 == ngr && cls.size() % 4 != 0) key[gi].first = 2.0;
    }
    std::stable_sort(key.begin(), key.end(), [](const std::pair<double, size_t>& a, const std::pair<double, size_t>& b) { return a.first < b.first; });
    std::vector<LatClass> out;
    out.reserve(cls.size());
    for (const auto& kv : key)
      for (size_t ci = kv.second * 4; ci < std::min(kv.second * 4 + 4, cls.size()); ++ci) out.push_back(std::move(cls[ci]));
    cls.swap(out);
  }
  ct.ncls = (int64_t)cls.size();
  ct.ngroups = (ct.ncls + 3) / 4;
  ct.xc.assign((size_t)(ct.ngroups + 1) * 4, 0.0);
  ct.gbatch0.assign((size_t)ct.ngroups + 1, 0);
  ct.cnt.assign((size_t)ct.ngroups * 8, 0.0);
  ct.crow.clear();
  const double d2r = M_PI / 180.0;
  for (int64_t gi = 0; gi < ct.ngroups; ++gi) {
    int bN = 0, bS = 0;
    for (int k = 0; k < 4; ++k) {
      const int64_t ci = gi * 4 + k;
      if (ci >= ct.ncls) continue;
      bN = std::max(bN, nb(cls[(size_t)ci].n.size()));
      bS = std::max(bS, nb(cls[(size_t)ci].s.size()));
      ct.xc[(size_t)ci] = std::cos((90.0 - cls[(size_t)ci].alat) * d2r);
      ct.cnt[(size_t)gi * 8 + k] = (double)cls[(size_t)ci].n.size();
      ct.cnt[(size_t)gi * 8 + 4 + k] = (double)cls[(size_t)ci].s.size();
    }
    ct.gbatch0[(size_t)gi] = (int)(ct.crow.size() / (4 * MB));
    for (int side = 0; side < 2; ++side) {
      const int nbat = side ? bS : bN;
      for (int bi = 0; bi < nbat; ++bi) {
        int flags = side ? CLS_SOUTH : 0;
        if (bi == 0 && (side == 0 || bN == 0)) flags |= CLS_FIRST;
        if (bi == nbat - 1 && (side == 1 || bS == 0)) flags |= CLS_LAST;
        int batch[4 * MB];
        bool haspad = false;
        for (int k = 0; k < 4; ++k) {
          const int64_t ci = gi * 4 + k;
          for (int j = 0; j < MB; ++j) {
            const size_t m = (size_t)bi * MB + j;
            int ent = (int)0x80000000 | (flags << 28);
            if (ci < ct.ncls) {
              const std::vector<int>& mem = side ? cls[(size_t)ci].s : cls[(size_t)ci].n;
              if (m < mem.size()) ent = mem[m] | (flags << 28);
            }
            haspad = haspad || ent < 0;
            batch[k * MB + j] = ent;
          }
        }
        for (int e = 0; e < 4 * MB; ++e) ct.crow.push_back(batch[e] | (haspad ? CLS_HASPAD_BIT : 0));
      }
    }
  }
  ct.nbatch = (int64_t)(ct.crow.size() / (4 * MB));
  ct.gbatch0[(size_t)ct.ngroups] = (int)ct.nbatch;
  ct.crow.resize(ct.crow.size() + (size_t)CLS_PADB * 4 * MB, (int)0x80000000);   // index loads run ahead
  return true;
}

// ---- work cuts ----------------------------------------------------------------------------------------------------
// (first batch, its group) of `nsub` pieces of the batch list, nsub + 1 pairs.  gbatch0[ngroups + 1] is the first batch
// of every class-group (+ total), of the full table or of a subsample.  Plain cuts have equal batch counts and may fall
// inside a class-group (the sweeps are linear in the member rows, the kernels project partial sums).  Group-aligned
// cuts (the sweeps that store whole-class sums) fall on the next group boundary and balance batches +
// TEMX_GROUP_COST per class-group: the end of a group (exchange, reference, 100-160 MFMAs) costs about two batches, and
// the table ends with the small classes (ne240: 361 groups of 2 batches), so that cuts by batch count alone gave the
// last workgroup twice the groups -- 1.9 instead of 1.5 ms for ne240 x 128 x 1
// (profiles/r03_lab20_class_order_d128_f32.log)
#ifndef TEMX_GROUP_COST
#define TEMX_GROUP_COST 2
#endif
inline std::vector<int> work_cuts(const std::vector<int>& gbatch0, int64_t ngroups, int64_t nbatches, int nsub, bool group_aligned) {
  std::vector<int> cut((size_t)2 * (nsub + 1));
  int g = 0;
  const int64_t total = nbatches + (int64_t)TEMX_GROUP_COST * ngroups;
  for (int k = 0; k <= nsub; ++k) {
    const int64_t b = nbatches * k / nsub;
    if (group_aligned) {
      const int64_t want = total * k / nsub;
      while (g < ngroups && gbatch0[(size_t)g] + (int64_t)TEMX_GROUP_COST * g < want) ++g;
      if (k == nsub) g = (int)ngroups;
      cut[(size_t)2 * k] = gbatch0[(size_t)g];
      cut[(size_t)2 * k + 1] = g;
      continue;
    }
    while (g + 1 < ngroups && gbatch0[(size_t)g + 1] <= b) ++g;
    cut[(size_t)2 * k] = (int)b;
    cut[(size_t)2 * k + 1] = g;
  }
  return cut;
}

// ---- subsample of class-groups (reference pre-pass of the single sweep, kernels_op2.hpp) --------------------------
// Every S-th group of the table with its batches copied, S = groups / keep (at most 256): 32 class-groups = 128
// latitudes for the 16 coefficients of a column -- the fit only has to be decent, it is removed again exactly; 96
// groups cost 0.15 instead of 0.06 ms at ne120 x 72 x 30 and 0.5 instead of 0.2 ms at ne30 x 72 x 91.
struct ClassSubsample {
  int64_t S = 1, ngroups = 0, nbatch = 0;
  std::vector<int> crow;        // [nbatch + CLS_PADB][4][CLS_MB]
  std::vector<double> xc;       // [4 * (ngroups + 1)]
  std::vector<int> gbatch0;     // [ngroups + 1]
};

inline ClassSubsample class_subsample(const std::vector<int>& crow, const std::vector<double>& xc, const std::vector<int>& gbatch0,
                                      int64_t ngroups, int64_t keep) {
  constexpr size_t per = 4 * CLS_MB;
  ClassSubsample ss;
  ss.S = std::max<int64_t>(1, std::min<int64_t>(256, ngroups / keep));
  for (int64_t gi = 0; gi < ngroups; gi += ss.S) {
    ss.gbatch0.push_back((int)(ss.crow.size() / per));
    ss.crow.insert(ss.crow.end(), crow.begin() + (size_t)gbatch0[(size_t)gi] * per, crow.begin() + (size_t)gbatch0[(size_t)gi + 1] * per);
    ss.xc.insert(ss.xc.end(), xc.begin() + (size_t)gi * 4, xc.begin() + (size_t)gi * 4 + 4);
  }
  ss.ngroups = (int64_t)ss.gbatch0.size();
  ss.nbatch = (int64_t)(ss.crow.size() / per);
  ss.gbatch0.push_back((int)ss.nbatch);
  ss.crow.resize(ss.crow.size() + (size_t)CLS_PADB * per, (int)0x80000000);   // index loads run ahead
  ss.xc.resize(ss.xc.size() + 4, 0.0);     // classes beyond the real ones have count 0 and x = 0: harmless rows
  return ss;
}

}  // namespace temx

#endif
