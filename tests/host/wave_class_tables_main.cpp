// The host tables of the class form of the zonal-wavenumber fit (pytemdiags_amd/csrc/wave_class_tables.hpp) on their
// own: the header needs no HIP.  usage: wave_class_tables_main GRID SIDE_CAP M...
// GRID is a text file "N" then N lines "lat_deg lon_deg"; SIDE_CAP the cut of long class sides of a plan made for fp32
// fields (0: none); M... the wavenumbers.  Builds the plan's class tables (build_classes) and checks, for every M:
// each member entry of the row table carries cos and sin of M times its OWN longitude, padding entries and the padding
// batches behind the table carry zeros, every column is a member exactly once; then that each class side has exactly
// one representative, a member of that side, and a side without members none; that the block layout of a class-group's
// table round-trips (every degree and column of every instantiation has a slot of its own inside the group's run, and
// the accumulator map leads back to it); the shape arithmetic for every (L, m) the form serves; and the count of cuts
// inside a class-group against the definition.  Prints "N=<n> classes=<n> groups=<n> batches=<n> max_side=<n>
// weights=ok reps=ok layout=ok shapes=<n> cuts=ok"; a failed check prints the case and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../pytemdiags_amd/csrc/wave_class_tables.hpp"

static int bad(const char* what, long long a, long long b) {
  std::printf("FAILED %s (%lld, %lld)\n", what, a, b);
  return 1;
}

int main(int argc, char** argv) {
  using namespace temx;
  if (argc < 4) return bad("usage", argc, 0);
  FILE* fh = std::fopen(argv[1], "r");
  if (!fh) return bad("open", 0, 0);
  long long N = 0;
  if (std::fscanf(fh, "%lld", &N) != 1 || N < 1) return bad("header", N, 0);
  std::vector<double> lat((size_t)N), lon((size_t)N), lon_rad((size_t)N);
  for (long long i = 0; i < N; ++i) {
    if (std::fscanf(fh, "%lf %lf", &lat[(size_t)i], &lon[(size_t)i]) != 2) return bad("row", i, 0);
    lon_rad[(size_t)i] = lon[(size_t)i] * M_PI / 180.0;
  }
  std::fclose(fh);
  const size_t cap = (size_t)std::atoi(argv[2]);
  const double tol = cap ? 1e-8 : 1e-11;
  ClassTables ct;
  if (!build_classes(lat.data(), N, ct, tol, cap, TEMX_F32_SIDE_KEEP)) return bad("build_classes", N, (long long)cap);
  constexpr int MB = CLS_MB;
  const size_t per = 4 * MB;
  if (ct.crow.size() != (size_t)(ct.nbatch + CLS_PADB) * per) return bad("row table size", (long long)ct.crow.size(), ct.nbatch);

  // ---- weights ----
  for (int a = 3; a < argc; ++a) {
    const int m = std::atoi(argv[a]);
    const std::vector<double> w = wavecls_weights(ct.crow, lon_rad.data(), m);
    if (w.size() != 2 * ct.crow.size()) return bad("weights size", m, (long long)w.size());
    std::vector<int> seen((size_t)N, 0);
    for (size_t e = 0; e < ct.crow.size(); ++e) {
      const int ent = ct.crow[e];
      if (ent < 0 || e >= (size_t)ct.nbatch * per) {
        if (ent >= 0) return bad("padding batch holds a member", m, (long long)e);
        if (w[2 * e] != 0.0 || w[2 * e + 1] != 0.0) return bad("padding weighs nothing", m, (long long)e);
        continue;
      }
      const int row = ent & WAVECLS_ROWMASK;
      if (row >= N) return bad("row in range", m, row);
      ++seen[(size_t)row];
      const double ang = (double)m * lon_rad[(size_t)row];
      if (w[2 * e] != std::cos(ang) || w[2 * e + 1] != std::sin(ang)) return bad("entry carries its own longitude", m, (long long)e);
      if (std::fabs(w[2 * e] * w[2 * e] + w[2 * e + 1] * w[2 * e + 1] - 1.0) > 1e-15) return bad("unit weights", m, (long long)e);
    }
    for (long long i = 0; i < N; ++i)
      if (seen[(size_t)i] != 1) return bad("every column is a member once", i, seen[(size_t)i]);
  }

  // ---- representatives ----
  const std::vector<int> rep = wavecls_representatives(ct.crow, ct.gbatch0, ct.ngroups);
  if (rep.size() != (size_t)(ct.ngroups + 1) * 8) return bad("representatives size", (long long)rep.size(), ct.ngroups);
  // the members of every class side, from the table itself
  std::vector<std::set<int>> members((size_t)(ct.ngroups + 1) * 8);
  for (long long gi = 0; gi < ct.ngroups; ++gi)
    for (int b = ct.gbatch0[(size_t)gi]; b < ct.gbatch0[(size_t)gi + 1]; ++b)
      for (int k = 0; k < 4; ++k)
        for (int j = 0; j < MB; ++j) {
          const int ent = ct.crow[((size_t)b * 4 + k) * MB + j];
          if (ent >= 0) members[((size_t)gi * 4 + k) * 2 + ((ent >> 28) & CLS_SOUTH)].insert(ent & WAVECLS_ROWMASK);
        }
  for (size_t ci = 0; ci < (size_t)(ct.ngroups + 1) * 4; ++ci)
    for (int side = 0; side < 2; ++side) {
      const std::set<int>& mem = members[ci * 2 + side];
      const int r = rep[ci * 2 + side];
      const double want = ci < (size_t)ct.ncls ? ct.cnt[(ci >> 2) * 8 + side * 4 + (ci & 3)] : 0.0;
      if ((double)mem.size() != want) return bad("member count of a side", (long long)ci, side);
      if (mem.empty() ? r != -1 : mem.count(r) != 1) return bad("one representative per class side", (long long)ci, side);
      if (r < 0) continue;
      if (side ? !(lat[(size_t)r] < 0.0) : !(lat[(size_t)r] >= -tol)) return bad("representative on its side", (long long)ci, side);
      const double xc = std::sin(std::fabs(lat[(size_t)r]) * M_PI / 180.0);
      if (std::fabs(xc - ct.xc[ci]) > 1e-9) return bad("representative at the class latitude", (long long)ci, side);
    }

  // ---- block layout ----
  for (int TBS : {2, 4, 7, 8}) {
    const int TE = wavecls_group_doubles(TBS);
    if (TE != 10 * TBS * 16 || wavecls_basis_doubles(TBS) != 2 * TBS * 16 || wavecls_defl_doubles(TBS) != 4 * TBS * 16)
      return bad("group size", TBS, TE);
    for (int ndeg = 1; ndeg <= 8 * TBS && ndeg <= WAVECLS_NDEG_MAX; ++ndeg) {
      std::set<int> used;
      for (int k = 0; k < 4; ++k) {
        for (int r = 0; r < ndeg; ++r) {
          const int s = wavecls_basis_slot(TBS, r, k);
          if (s < 0 || s >= wavecls_basis_doubles(TBS) || !used.insert(s).second) return bad("basis slot", TBS, r);
          if ((s % 16) / 4 != k) return bad("basis slot holds its class", TBS, r);
          const int t = s / 16, i = s % 4;
          if (wavecls_acc_col(TBS, ndeg, t, i) != r || wavecls_acc_col(TBS, ndeg, 2 * TBS + t, i) != ndeg + r)
            return bad("basis round trip", TBS, r);
          if ((t >= TBS) != ((r & 1) == 1)) return bad("parity of a basis block", TBS, r);
        }
        for (int which = 0; which < 2; ++which)
          for (int j = 0; j < 2 * ndeg; ++j) {
            const int s = wavecls_defl_slot(TBS, ndeg, j, k, which);
            if (s < wavecls_basis_doubles(TBS) || s >= TE || !used.insert(s).second) return bad("deflation slot", TBS, j);
            const int o = s - wavecls_basis_doubles(TBS) - which * wavecls_defl_doubles(TBS);
            if (o < 0 || o >= wavecls_defl_doubles(TBS)) return bad("deflation slot in its table", TBS, j);
            if ((o % 16) / 4 != k || wavecls_acc_col(TBS, ndeg, o / 16, o % 4) != j) return bad("deflation round trip", TBS, j);
          }
      }
      // every accumulator element is a column or padding, and every column is met once
      int cols = 0;
      for (int a = 0; a < 4 * TBS; ++a)
        for (int i = 0; i < 4; ++i) {
          const int j = wavecls_acc_col(TBS, ndeg, a, i);
          if (j < -1 || j >= 2 * ndeg) return bad("accumulator column", TBS, a);
          cols += j >= 0;
        }
      if (cols != 2 * ndeg) return bad("accumulators cover the basis once", TBS, ndeg);
    }
  }

  // ---- shapes ----
  long long shapes = 0;
  for (int L = 1; L <= 511; ++L)
    for (int m = 1; m <= L; ++m) {
      if (L + 1 - m > WAVECLS_NDEG_MAX) continue;
      const WaveClsShape s = wavecls_shape(L, m);
      ++shapes;
      if (s.ndeg != L + 1 - m || s.Kc != 2 * s.ndeg || s.nacc != 4 * s.TBS || s.fpw != 1) return bad("shape", L, m);
      if (s.TBS != 2 && s.TBS != 4 && s.TBS != 7 && s.TBS != 8) return bad("instantiation", L, m);
      if (8 * s.TBS < s.ndeg) return bad("blocks hold the degrees", L, m);
      if (s.TBS > 2 && 8 * (s.TBS == 8 ? 7 : (s.TBS == 7 ? 4 : 2)) >= s.ndeg + (s.ndeg & 1)) return bad("smallest instantiation", L, m);
    }
  if (wavecls_shape(50, 1).TBS != 7 || wavecls_shape(64, 1).TBS != 8 || wavecls_shape(20, 20).TBS != 2) return bad("known shapes", 0, 0);

  // ---- cuts inside a class-group ----
  for (int nsub : {1, 2, 3, 7, 16, 61}) {
    if (nsub > ct.nbatch) continue;
    const std::vector<int> cut = work_cuts(ct.gbatch0, ct.ngroups, ct.nbatch, nsub, false);
    int inside = 0;
    for (int k = 1; k < nsub; ++k) {
      const int b = cut[(size_t)2 * k];
      bool at_start = false;
      for (long long gi = 0; gi <= ct.ngroups; ++gi) at_start = at_start || ct.gbatch0[(size_t)gi] == b;
      inside += !at_start;
    }
    if (wavecls_cuts_inside(ct.gbatch0, ct.ngroups, ct.nbatch, nsub) != inside) return bad("cuts inside a group", nsub, inside);
    if (nsub == 1 && inside != 0) return bad("one piece has no cut", nsub, inside);
  }

  std::printf("N=%lld classes=%lld groups=%lld batches=%lld max_side=%lld weights=ok reps=ok layout=ok shapes=%lld cuts=ok\n", N,
              (long long)ct.ncls, (long long)ct.ngroups, (long long)ct.nbatch, (long long)ct.max_side, shapes);
  return 0;
}
