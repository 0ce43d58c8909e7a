// The launch shapes of the time sum over valid times (nclim_shape, pytemdiags_amd/csrc/nclim_shapes.hpp) on their own:
// the header needs no HIP.  usage: nclim_shapes_main nt_max
// For every nt in 1..nt_max, both element sizes, nf = 1..8, both mask modes and a few row counts it walks the launch
// the way the kernels do and checks that every row is owned exactly once (staged: by one workgroup, at one LDS row, by
// one group of g lanes inside one wave; long: by one wave), that the staged images of the fields a workgroup holds are
// disjoint and inside the LDS budget, and that the kernel changes exactly at nclim_switch_nt.  Prints one line
// "switch esz=<e> nfs=<n> nt=<nt>" per (element size, fields per workgroup) and "cases=<n>"; a failed check prints
// the case and exits 1.  tests/test_nclim_host.py builds it with AddressSanitizer + UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pytemdiags_amd/csrc/nclim_shapes.hpp"

static int bad(const char* what, long long rows, long long nt, int esz, int nf, int common) {
  std::printf("FAILED %s rows=%lld nt=%lld esz=%d nf=%d common=%d\n", what, rows, nt, esz, nf, common);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const long long nt_max = std::atoll(argv[1]);
  const long long row_counts[] = {1, 37, 257, 1031};
  long long cases = 0;
  for (int esz : {8, 4})
    for (int common : {0, 1})
      for (int nf = 1; nf <= temx::NCLIM_NFMAX; ++nf) {
        const int nfs = common ? nf : 1;       // fields a workgroup holds
        const int64_t sw = temx::nclim_switch_nt((size_t)esz, nfs);
        if (nf == 1 || common) std::printf("switch esz=%d nfs=%d nt=%" PRId64 "\n", esz, nfs, sw);
        for (long long nt = 1; nt <= nt_max; ++nt)
          for (long long rows : row_counts) {
            const temx::NclimShape s = temx::nclim_shape(rows, nt, (size_t)esz, nfs);
            ++cases;
            if ((s.staged != 0) != (nt < sw)) return bad("switch point", rows, nt, esz, nf, common);
            if (s.rpb < 1 || s.nblk != (rows + s.rpb - 1) / s.rpb) return bad("workgroup count", rows, nt, esz, nf, common);
            std::vector<int> owned((size_t)rows, 0);
            if (s.staged) {
              if (!(s.stride & 1) || s.stride < nt) return bad("stride", rows, nt, esz, nf, common);
              const long long img = (long long)s.rpb * s.stride;
              if (nfs * img * esz > temx::NCLIM_LDS_BYTES) return bad("LDS budget", rows, nt, esz, nf, common);
              if (s.rpb < temx::NCLIM_MIN_ROWS || s.rpb > temx::NCLIM_THREADS) return bad("rows per workgroup", rows, nt, esz, nf, common);
              if (s.g < 1 || s.g > 64 || (s.g & (s.g - 1)) || s.rpb * s.g > temx::NCLIM_THREADS)
                return bad("lanes per row", rows, nt, esz, nf, common);
              std::vector<char> image((size_t)(temx::NCLIM_LDS_BYTES / esz), 0);
              for (int64_t b = 0; b < s.nblk; ++b) {
                const int64_t r0 = b * s.rpb;
                const int nr = (int)(rows - r0 < s.rpb ? rows - r0 : s.rpb);
                if (b == 0)                                 // the images of a workgroup: no two elements share a slot
                  for (int f = 0; f < nfs; ++f)
                    for (int r = 0; r < nr; ++r)
                      for (long long t = 0; t < nt; ++t) {
                        char& c = image.at((size_t)(f * img) + (size_t)r * s.stride + (size_t)t);
                        if (c) return bad("LDS slot used twice", rows, nt, esz, nf, common);
                        c = 1;
                      }
                for (int tid = 0; tid < temx::NCLIM_THREADS; ++tid) {
                  const int r = tid / s.g, j = tid - r * s.g;
                  if (b == 0 && (tid >> 6) != ((r * s.g) >> 6)) return bad("row across waves", rows, nt, esz, nf, common);
                  if (r < nr && j == 0) ++owned.at((size_t)(r0 + r));
                }
              }
            } else {
              if (s.rpb != temx::NCLIM_LONG_ROWS) return bad("rows per workgroup", rows, nt, esz, nf, common);
              for (int64_t b = 0; b < s.nblk; ++b)
                for (int w = 0; w < temx::NCLIM_LONG_ROWS; ++w) {
                  const int64_t row = b * temx::NCLIM_LONG_ROWS + w;
                  if (row < rows) ++owned.at((size_t)row);
                }
            }
            for (int c : owned)
              if (c != 1) return bad("row not owned exactly once", rows, nt, esz, nf, common);
          }
      }
  std::printf("cases=%lld\n", cases);
  return 0;
}
