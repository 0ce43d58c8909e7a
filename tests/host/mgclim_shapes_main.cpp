// The launch shapes of the masked grouped time sum (mgclim_shape, pytemdiags_amd/csrc/mgclim_shapes.hpp) on their own:
// the header needs no HIP.  usage: mgclim_shapes_main nt_max
// For every nt in 1..nt_max, both element sizes, 1..8 fields per workgroup (own-mask mode is one field per workgroup
// whatever nf), 1..64 groups present and a few row counts it walks the launch the way the kernels do and checks that
// every (row, group present) unit is owned exactly once (staged: by one lane of one workgroup in one round; long rows:
// by one wave, in one pass, at one slot), that the staged images stay inside NCLIM_LDS_BYTES and the images of a
// workgroup's waves inside MGCLIM_LONG_LDS_BYTES, that the batches partition the groups present, and that the form
// changes exactly at mgclim_switch_nt (staged / long) and at gclim_bound (registers / LDS).  Ownership is walked at
// EVERY nt (the staged rows per workgroup change with every nt): at every row count and every np for nt <= 16, every
// 37th nt, the nt at and after every multiple of 64 and the five around the switch; at 37 rows and np in {1, 5, 64} for
// every other nt, which also checks the shape's own invariants for every np.  Then the argument rules of the entry point
// (check_sum_groups_valid of field_args.hpp) on made-up addresses: every refusal and the well-formed calls next to it.
// Prints "switch esz=<e> nt=<nt>" per element size, "batch nfs=<n> slots=<b>" per number of fields, "cases=<n>
// walked=<n>" and "refusals=<n>"; a failed check prints the case and exits 1.  tests/test_mgclim_host.py builds it with
// AddressSanitizer + UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pytemdiags_amd/csrc/field_args.hpp"
#include "../../pytemdiags_amd/csrc/mgclim_shapes.hpp"

// check_sum_groups_valid on made-up addresses: src of 60 fp64 (480 bytes) at 4096, outputs of 24 doubles (192 bytes)
static int refusals_of_the_entry_point(int* count) {
  using namespace temx;
  auto P = [](uintptr_t a) { return reinterpret_cast<double*>(a); };
  const void* src1[1] = {reinterpret_cast<const void*>(uintptr_t(4096))};
  const void* src2[2] = {src1[0], reinterpret_cast<const void*>(uintptr_t(8192))};
  const uintptr_t A = 1 << 20, W = 2 << 20, C = 3 << 20;
  struct Case { int nf; uintptr_t acc[2], wsum[2], cnt[2]; int nextra; int dtype; uintptr_t src0; const char* want; };
  const Case cases[] = {
      {1, {A, 0}, {W, 0}, {C, 0}, 1, TEMX_F64, 4096, nullptr},
      {1, {A, 0}, {A + 192, 0}, {A + 384, 0}, 1, TEMX_F64, 4096, nullptr},                 // touching is fine
      {1, {4096 + 480, 0}, {4096 - 192, 0}, {C, 0}, 1, TEMX_F64, 4096, nullptr},
      {1, {A, 0}, {W, 0}, {C, 0}, 1, TEMX_F32, 4100, nullptr},                             // fp32 at 4 mod 8 is aligned
      {1, {A, 0}, {W, 0}, {C, 0}, 1, TEMX_F64, 4100, "src 0 is not aligned"},
      {1, {0, 0}, {W, 0}, {C, 0}, 1, TEMX_F64, 4096, "acc 0 is null"},
      {1, {A, 0}, {0, 0}, {C, 0}, 1, TEMX_F64, 4096, "wsum 0 is null"},
      {1, {A, 0}, {W, 0}, {0, 0}, 1, TEMX_F64, 4096, "cnt 0 is null"},
      {1, {A + 4, 0}, {W, 0}, {C, 0}, 1, TEMX_F64, 4096, "acc 0 is not aligned"},
      {1, {A, 0}, {W + 4, 0}, {C, 0}, 1, TEMX_F64, 4096, "wsum 0 is not aligned"},
      {1, {A, 0}, {W, 0}, {C + 4, 0}, 1, TEMX_F64, 4096, "cnt 0 is not aligned"},
      {1, {4096 + 472, 0}, {W, 0}, {C, 0}, 1, TEMX_F64, 4096, "acc 0 overlaps src 0"},
      {1, {A, 0}, {4096 - 184, 0}, {C, 0}, 1, TEMX_F64, 4096, "wsum 0 overlaps src 0"},
      {1, {A, 0}, {W, 0}, {4096 + 472, 0}, 1, TEMX_F64, 4096, "cnt 0 overlaps src 0"},
      {1, {A, 0}, {A + 184, 0}, {C, 0}, 1, TEMX_F64, 4096, "wsum 0 overlaps acc 0"},
      {1, {A, 0}, {W, 0}, {A - 184, 0}, 1, TEMX_F64, 4096, "cnt 0 overlaps acc 0"},
      {1, {A, 0}, {C + 8, 0}, {C, 0}, 1, TEMX_F64, 4096, "wsum 0 overlaps cnt 0"},
      {2, {A, A + 192}, {W, 0}, {C, 0}, 1, TEMX_F64, 4096, nullptr},                       // common mask: [0] only
      {2, {A, A + 184}, {W, 0}, {C, 0}, 1, TEMX_F64, 4096, "acc 1 overlaps acc 0"},
      {2, {A, A + 192}, {W, W + 192}, {C, C + 192}, 2, TEMX_F64, 4096, nullptr},
      {2, {A, A + 192}, {W, 0}, {C, C + 192}, 2, TEMX_F64, 4096, "wsum 1 is null"},
      {2, {A, A + 192}, {W, W + 192}, {C, 0}, 2, TEMX_F64, 4096, "cnt 1 is null"},
      {2, {A, A + 192}, {W, W + 184}, {C, C + 192}, 2, TEMX_F64, 4096, "wsum 1 overlaps wsum 0"},
      {2, {A, A + 192}, {W, W + 192}, {C, C + 184}, 2, TEMX_F64, 4096, "cnt 1 overlaps cnt 0"},
      {2, {A, A + 192}, {W, 8192 + 472}, {C, C + 192}, 2, TEMX_F64, 4096, "wsum 1 overlaps src 1"},
      {2, {A, A + 192}, {W, C + 200}, {C, C + 192}, 2, TEMX_F64, 4096, "wsum 1 overlaps cnt 1"},
  };
  for (const Case& c : cases) {
    const void* src[2] = {reinterpret_cast<const void*>(c.src0), src2[1]};
    double* acc[2] = {P(c.acc[0]), P(c.acc[1])};
    double* wsum[2] = {P(c.wsum[0]), P(c.wsum[1])};
    double* cnt[2] = {P(c.cnt[0]), P(c.cnt[1])};
    const Refusal r = check_sum_groups_valid(c.nf, src, c.dtype, 60, acc, wsum, cnt, c.nextra, 24);
    const bool ok = c.want ? (r.code == TEMX_EINVAL && std::strstr(r.msg, c.want)) : (r.code == TEMX_OK);
    if (!ok) {
      std::printf("FAILED refusal: wanted \"%s\", got %d \"%s\"\n", c.want ? c.want : "(accepted)", r.code, r.msg);
      return 1;
    }
    *count += c.want ? 1 : 0;
  }
  return 0;
}

static int bad(const char* what, long long rows, long long nt, int esz, int nfs, int np) {
  std::printf("FAILED %s rows=%lld nt=%lld esz=%d nfs=%d np=%d\n", what, rows, nt, esz, nfs, np);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  using namespace temx;
  const long long nt_max = std::atoll(argv[1]);
  const long long row_counts[] = {1, 37, 257};
  long long cases = 0, walked = 0;
  for (int nfs = 1; nfs <= MGCLIM_NFMAX; ++nfs) std::printf("batch nfs=%d slots=%d\n", nfs, mgclim_batch(nfs));
  for (int common : {0, 1})
    for (int nf = 1; nf <= MGCLIM_NFMAX; ++nf) {
      if (mgclim_nfs(nf, common != 0) != (common ? nf : 1)) return bad("fields per workgroup", 0, 0, 0, nf, common);
      if (mgclim_nft(nf, common != 0) < mgclim_nfs(nf, common != 0)) return bad("instantiation", 0, 0, 0, nf, common);
    }
  for (int esz : {8, 4}) {
    const int64_t sw = mgclim_switch_nt((size_t)esz);
    std::printf("switch esz=%d nt=%" PRId64 "\n", esz, sw);
    if (sw != clim_switch_nt((size_t)esz)) return bad("switch is not the grouped sum's", 0, sw, esz, 0, 0);
    for (int nfs = 1; nfs <= MGCLIM_NFMAX; ++nfs)
      for (long long nt = 1; nt <= nt_max; ++nt) {
        const bool walk = nt <= 16 || nt % 64 < 2 || nt % 37 == 0 || (nt >= sw - 2 && nt <= sw + 2);
        for (int np = 1; np <= MGCLIM_NGMAX; ++np)
          for (long long rows : row_counts) {
            if (!walk && rows != 37) continue;
            const bool own = walk || np == 1 || np == 5 || np == MGCLIM_NGMAX;   // ownership is walked for this case
            const MgclimShape s = mgclim_shape(rows, nt, (size_t)esz, nfs, np);
            ++cases;
            walked += own ? 1 : 0;
            if ((s.staged != 0) != (nt < sw)) return bad("switch point", rows, nt, esz, nfs, np);
            if (s.rpw < 1 || s.nblk != (rows + s.rpw - 1) / s.rpw) return bad("workgroup count", rows, nt, esz, nfs, np);
            std::vector<int> owned(own ? (size_t)rows * (size_t)np : 0, 0);
            if (s.staged) {
              if (!(s.stride & 1) || s.stride < nt) return bad("stride", rows, nt, esz, nfs, np);
              if (nt >= MGCLIM_STAGED_NT) return bad("the table's LDS copy holds the window", rows, nt, esz, nfs, np);
              if (s.rpb != s.rpw || s.rpb > MGCLIM_THREADS) return bad("rows per workgroup", rows, nt, esz, nfs, np);
              if (s.lds_bytes != (size_t)nfs * s.rpb * s.stride * esz || s.lds_bytes > (size_t)NCLIM_LDS_BYTES)
                return bad("staged bytes", rows, nt, esz, nfs, np);
              const NclimShape n = nclim_shape(rows, nt, (size_t)esz, nfs);     // where that shape stages, this is it
              if (n.staged ? (s.rpb != n.rpb || s.stride != n.stride) : (s.rpb >= NCLIM_MIN_ROWS || s.rpb < 2))
                return bad("not built on nclim_shape", rows, nt, esz, nfs, np);
              if (s.bound != 0 || s.batch != 0 || s.npass != 1) return bad("staged form fields", rows, nt, esz, nfs, np);
              if (!own) continue;
              for (int64_t b = 0; b < s.nblk; ++b) {
                const int64_t r0 = b * s.rpb;
                const int nr = (int)(rows - r0 < s.rpb ? rows - r0 : s.rpb);
                const int units = np * nr;
                for (int tid = 0; tid < MGCLIM_THREADS; ++tid)
                  for (int u = tid; u < units; u += MGCLIM_THREADS) {
                    int q, r;
                    mgclim_unit(u, nr, &q, &r);
                    if (q < 0 || q >= np || r < 0 || r >= nr) return bad("unit out of range", rows, nt, esz, nfs, np);
                    ++owned.at((size_t)(r0 + r) * np + (size_t)q);
                  }
              }
            } else {
              if (s.bound != gclim_bound(np)) return bad("form of the long rows", rows, nt, esz, nfs, np);
              if ((s.bound == GCLIM_NGMAX) != (np > 4)) return bad("register / LDS switch", rows, nt, esz, nfs, np);
              if (s.bound != GCLIM_NGMAX) {
                if (s.rpw != NCLIM_LONG_ROWS || s.batch != 0 || s.npass != 1 || s.lds_bytes != 0)
                  return bad("register form fields", rows, nt, esz, nfs, np);
              } else {
                const int cap = mgclim_batch(nfs);
                if (cap < 1 || cap * mgclim_slot_bytes(nfs) > MGCLIM_LONG_LDS_BYTES ||
                    (cap + 1) * mgclim_slot_bytes(nfs) <= MGCLIM_LONG_LDS_BYTES)
                  return bad("batch is not the largest that fits", rows, nt, esz, nfs, np);
                if (s.batch != (np < cap ? np : cap) || s.npass != (np + s.batch - 1) / s.batch)
                  return bad("batches", rows, nt, esz, nfs, np);
                if (s.rpw > NCLIM_LONG_ROWS || s.lds_bytes != (size_t)s.rpw * s.batch * mgclim_slot_bytes(nfs) ||
                    s.lds_bytes > (size_t)MGCLIM_LONG_LDS_BYTES)
                  return bad("LDS image", rows, nt, esz, nfs, np);
                if (s.rpw < NCLIM_LONG_ROWS && (size_t)(s.rpw + 1) * s.batch * mgclim_slot_bytes(nfs) <= (size_t)MGCLIM_LONG_LDS_BYTES)
                  return bad("more waves would fit", rows, nt, esz, nfs, np);
              }
              if (!own) continue;
              const int batch = s.bound == GCLIM_NGMAX ? s.batch : np;
              for (int64_t b = 0; b < s.nblk; ++b)
                for (int w = 0; w < s.rpw; ++w) {
                  const int64_t row = b * s.rpw + w;
                  if (row >= rows) continue;
                  int passes = 0;
                  for (int b0 = 0; b0 < np; b0 += batch, ++passes) {
                    const int nb = np - b0 < batch ? np - b0 : batch;
                    for (int sl = 0; sl < nb; ++sl) ++owned.at((size_t)row * np + (size_t)(b0 + sl));
                  }
                  if (passes != s.npass) return bad("passes", rows, nt, esz, nfs, np);
                }
            }
            for (int c : owned)
              if (c != 1) return bad("unit not owned exactly once", rows, nt, esz, nfs, np);
          }
      }
  }
  std::printf("cases=%lld walked=%lld\n", cases, walked);
  int refusals = 0;
  if (refusals_of_the_entry_point(&refusals)) return 1;
  std::printf("refusals=%d\n", refusals);
  return 0;
}
