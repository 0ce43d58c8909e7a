// The tables and launch shapes of the grouped time sum (pytemdiags_amd/csrc/gclim_tables.hpp) and its argument check
// (check_groups of field_args.hpp) on their own: neither header needs HIP.  usage: gclim_tables_main nt_record_max
// For every record length 1..nt_record_max, ng in {1, 2, 5, 12, 64}, random labels (about a tenth left out) and
// contiguous month-like labels, with and without weights, it builds the record's table and, for every window (t0, nt)
// of a few block sizes (every window at all while the record is short), the per-window part, and checks that
//   * every labelled time of the window appears in exactly one group's range, in ascending order, with its weight;
//   * left-out times and times outside the window appear in none;
//   * the list of groups present, their mask and their order are exact;
//   * the device image holds what the kernels read (weights, sorted weights, labels, sorted times);
//   * the staged bytes stay inside the LDS budget and the launch shape depends on (nt, element size, groups present) only.
// Prints "records=<n> windows=<n> refusals=<n>"; a failed check prints the case and exits 1.
// tests/test_gclim_host.py builds it with AddressSanitizer + UBSan.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../pytemdiags_amd/csrc/field_args.hpp"
#include "../../pytemdiags_amd/csrc/gclim_tables.hpp"

using namespace temx;

static int bad(const char* what, long long ntr, int ng, long long t0, long long nt) {
  std::printf("FAILED %s nt_record=%lld ng=%d t0=%lld nt=%lld\n", what, ntr, ng, t0, nt);
  return 1;
}

static int check_window(const GclimRecord& r, const std::vector<int32_t>& lab, const std::vector<double>& w, int64_t t0,
                        int64_t nt) {
  const long long ntr = (long long)r.nt_record;
  const GclimWindow win = gclim_window(r, t0, nt);
  const double* iw = reinterpret_cast<const double*>(r.image.data() + r.off_w());
  const double* isw = reinterpret_cast<const double*>(r.image.data() + r.off_sw());
  const int32_t* ist = reinterpret_cast<const int32_t*>(r.image.data() + r.off_st());
  std::vector<int> seen((size_t)r.nt_record, 0);
  unsigned long long mask = 0;
  if (win.ng != r.ng || win.np < 0 || win.np > r.ng) return bad("window header", ntr, r.ng, t0, nt);
  for (int q = 0; q < GCLIM_NGMAX; ++q) {
    if (q >= win.np) {
      if (win.pg[q] != -2) return bad("pg beyond np", ntr, r.ng, t0, nt);
      continue;
    }
    const int g = win.pg[q];
    if (g < 0 || g >= r.ng || (q && g <= win.pg[q - 1])) return bad("present list order", ntr, r.ng, t0, nt);
    if (win.lo[q] >= win.hi[q] || win.lo[q] < 0 || win.hi[q] > (int)r.sorted.size()) return bad("range", ntr, r.ng, t0, nt);
    mask |= 1ull << g;
    for (int j = win.lo[q]; j < win.hi[q]; ++j) {
      const int32_t t = ist[j];
      if (t < t0 || t >= t0 + nt) return bad("time outside the window", ntr, r.ng, t0, nt);
      if (lab[(size_t)t] != g) return bad("time in the wrong group", ntr, r.ng, t0, nt);
      if (j > win.lo[q] && t <= ist[j - 1]) return bad("times not ascending", ntr, r.ng, t0, nt);
      if (std::memcmp(&isw[j], &w[(size_t)t], 8) || std::memcmp(&iw[t], &w[(size_t)t], 8)) return bad("weight", ntr, r.ng, t0, nt);
      ++seen[(size_t)t];
    }
  }
  if (mask != win.mask) return bad("mask", ntr, r.ng, t0, nt);
  int present = 0;
  unsigned long long truth = 0;
  for (int64_t t = 0; t < r.nt_record; ++t) {
    const bool in = t >= t0 && t < t0 + nt && lab[(size_t)t] >= 0;
    if (seen[(size_t)t] != (in ? 1 : 0)) return bad(in ? "labelled time not owned exactly once" : "left-out time owned", ntr, r.ng, t0, nt);
    if (in) truth |= 1ull << lab[(size_t)t];
  }
  for (int g = 0; g < 64; ++g) present += (int)((truth >> g) & 1);
  if (truth != win.mask || present != win.np) return bad("groups present", ntr, r.ng, t0, nt);
  // launch shapes: inside the LDS budget, a function of (nt, element size, groups present) only
  if (win.np)
    for (size_t esz : {(size_t)8, (size_t)4}) {
      const GclimShape a = gclim_shape(1, nt, esz, win.np, r.ng), b = gclim_shape(866 * 6, nt, esz, win.np, r.ng);
      if (a.rows.staged != b.rows.staged || a.rows.rpb != b.rows.rpb || a.rows.stride != b.rows.stride || a.bound != b.bound ||
          a.lds_bytes != b.lds_bytes || a.rpw != b.rpw)
        return bad("shape depends on the rows", ntr, r.ng, t0, nt);
      if (a.nblk != 1 || b.nblk != (866 * 6 + b.rpw - 1) / b.rpw) return bad("workgroup count", ntr, r.ng, t0, nt);
      if (a.lds_bytes > (size_t)(a.rows.staged ? CLIM_LDS_BYTES : GCLIM_LONG_LDS_BYTES)) return bad("LDS budget", ntr, r.ng, t0, nt);
      if (a.rows.staged != (nt < clim_switch_nt(esz) ? 1 : 0)) return bad("switch point", ntr, r.ng, t0, nt);
      if (a.rows.staged ? (a.bound != 0 || a.rows.stride < nt || !(a.rows.stride & 1) || a.rpw != a.rows.rpb)
                        : (a.bound < win.np || (a.bound != 1 && a.bound != 4 && a.bound != 64) || a.rpw < 1 || a.rpw > CLIM_LONG_ROWS ||
                           (a.bound == 64 ? a.lds_bytes != (size_t)a.rpw * r.ng * 512 : (a.lds_bytes != 0 || a.rpw != CLIM_LONG_ROWS))))
        return bad("bound or stride", ntr, r.ng, t0, nt);
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const long long ntr_max = std::atoll(argv[1]);
  std::mt19937_64 rng(12345);
  long long records = 0, windows = 0, refusals = 0;
  for (long long ntr = 1; ntr <= ntr_max; ++ntr)
    for (int ng : {1, 2, 5, 12, 64})
      for (int kind = 0; kind < 2; ++kind) {
        std::vector<int32_t> lab((size_t)ntr);
        std::vector<double> w((size_t)ntr, 1.0);
        const bool weighted = ((ntr + ng + kind) % 3) != 0;
        for (long long t = 0; t < ntr; ++t) {
          if (kind == 0) lab[(size_t)t] = (rng() % 10 == 0) ? -1 : (int32_t)(rng() % (unsigned)ng);
          else lab[(size_t)t] = (int32_t)((t * ng) / ntr);     // contiguous, month-like
          if (weighted) w[(size_t)t] = (rng() % 7 == 0) ? 0.0 : 2.0 * (double)(rng() % 1000) / 999.0;
        }
        if (check_groups(ng, GCLIM_NGMAX, ntr, 0, ntr, lab.data(), weighted ? w.data() : nullptr))
          return bad("a good record was refused", ntr, ng, 0, ntr);
        const GclimRecord r = gclim_record(ng, ntr, lab.data(), weighted ? w.data() : nullptr);
        ++records;
        if (r.key != gclim_key(ng, ntr, lab.data(), weighted ? w.data() : nullptr)) return bad("key", ntr, ng, 0, ntr);
        if (r.image.size() != (size_t)ntr * 24 || (int)r.start.size() != ng + 1) return bad("image size", ntr, ng, 0, ntr);
        if (std::memcmp(r.image.data() + r.off_lab(), lab.data(), (size_t)ntr * 4)) return bad("labels of the image", ntr, ng, 0, ntr);
        if (ntr <= 40) {
          for (long long t0 = 0; t0 < ntr; ++t0)
            for (long long nt = 1; t0 + nt <= ntr; ++nt, ++windows)
              if (check_window(r, lab, w, t0, nt)) return 1;
        } else {
          for (long long blk : {1LL, 13LL, 64LL, ntr})
            for (long long t0 = 0; t0 < ntr; t0 += blk, ++windows)
              if (check_window(r, lab, w, t0, t0 + blk <= ntr ? blk : ntr - t0)) return 1;
        }
      }
  // ---- check_groups: what it refuses, and that it refuses nothing else ----
  {
    const int32_t lab[5] = {0, 1, -1, 2, 1};
    const double w[5] = {1, 0, 2, 0.5, 3};
    auto refused = [&](Refusal r, const char* word) {
      ++refusals;
      return r && r.code == TEMX_EINVAL && std::strstr(r.msg, word);
    };
    if (check_groups(3, 64, 5, 0, 5, lab, w) || check_groups(3, 64, 5, 2, 3, lab, nullptr) || check_groups(64, 64, 5, 4, 1, lab, w))
      return bad("a good call was refused", 5, 3, 0, 5);
    if (!refused(check_groups(0, 64, 5, 0, 5, lab, w), "ng") || !refused(check_groups(65, 64, 5, 0, 5, lab, w), "ng")) return bad("ng", 5, 0, 0, 5);
    if (!refused(check_groups(3, 64, 5, -1, 2, lab, w), "t0")) return bad("t0 < 0", 5, 3, -1, 2);
    if (!refused(check_groups(3, 64, 5, 3, 3, lab, w), "exceeds") || !refused(check_groups(3, 64, 5, 0, 6, lab, w), "exceeds"))
      return bad("window", 5, 3, 3, 3);
    if (!refused(check_groups(3, 64, 5, 0, 5, nullptr, w), "label_host")) return bad("null labels", 5, 3, 0, 5);
    if (!refused(check_groups(2, 64, 5, 0, 5, lab, w), "label 3")) return bad("label == ng", 5, 2, 0, 5);
    const int32_t low[2] = {0, -2};
    if (!refused(check_groups(3, 64, 2, 0, 2, low, nullptr), "label 1")) return bad("label -2", 2, 3, 0, 2);
    for (double v : {-1e-300, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()}) {
      double wb[5] = {1, 0, 2, v, 3};
      if (!refused(check_groups(3, 64, 5, 0, 5, lab, wb), "weight 3")) return bad("weight", 5, 3, 0, 5);
    }
  }
  std::printf("records=%lld windows=%lld refusals=%lld\n", records, windows, refusals);
  return 0;
}
