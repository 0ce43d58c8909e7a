// The launch shapes of the time sum (clim_shape, pytemdiags_amd/csrc/clim_shapes.hpp) on their own: the header needs no
// HIP.  usage: clim_shapes_main nt_max
// For every nt in 1..nt_max, both element sizes and a few row counts it walks the launch the way the kernels do and
// checks that every row is owned exactly once (staged: by one workgroup, at one LDS row, by one group of g lanes inside
// one wave; long: by one wave), that the staged image fits the LDS budget, and that the kernel changes exactly at
// clim_switch_nt.  Prints "switch_f64=<nt> switch_f32=<nt> cases=<n>"; a failed check prints the case and exits 1.
// tests/test_clim_host.py builds it with AddressSanitizer + UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pytemdiags_amd/csrc/clim_shapes.hpp"

static int bad(const char* what, long long rows, long long nt, int esz) {
  std::printf("FAILED %s rows=%lld nt=%lld esz=%d\n", what, rows, nt, esz);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const long long nt_max = std::atoll(argv[1]);
  const long long row_counts[] = {1, 3, 37, 255, 256, 257, 866 * 6, 4099};
  long long cases = 0;
  for (int esz : {8, 4}) {
    const int64_t sw = temx::clim_switch_nt((size_t)esz);
    for (long long nt = 1; nt <= nt_max; ++nt)
      for (long long rows : row_counts) {
        const temx::ClimShape s = temx::clim_shape(rows, nt, (size_t)esz);
        ++cases;
        if ((s.staged != 0) != (nt < sw)) return bad("switch point", rows, nt, esz);
        if (s.rpb < 1 || s.nblk != (rows + s.rpb - 1) / s.rpb) return bad("workgroup count", rows, nt, esz);
        std::vector<int> owned((size_t)rows, 0);
        if (s.staged) {
          if (!(s.stride & 1) || s.stride < nt) return bad("stride", rows, nt, esz);
          if ((long long)s.rpb * s.stride * esz > temx::CLIM_LDS_BYTES) return bad("LDS budget", rows, nt, esz);
          if (s.rpb < temx::CLIM_MIN_ROWS || s.rpb > temx::CLIM_THREADS) return bad("rows per workgroup", rows, nt, esz);
          if (s.g < 1 || s.g > 64 || (s.g & (s.g - 1)) || s.rpb * s.g > temx::CLIM_THREADS) return bad("lanes per row", rows, nt, esz);
          std::vector<char> image((size_t)(temx::CLIM_LDS_BYTES / esz), 0);
          for (int64_t b = 0; b < s.nblk; ++b) {
            const int64_t r0 = b * s.rpb;
            const int nr = (int)(rows - r0 < s.rpb ? rows - r0 : s.rpb);
            if (b == 0)                                     // the image of a workgroup: no two elements share a slot
              for (int r = 0; r < nr; ++r)
                for (long long t = 0; t < nt; ++t) {
                  char& c = image.at((size_t)r * s.stride + (size_t)t);
                  if (c) return bad("LDS slot used twice", rows, nt, esz);
                  c = 1;
                }
            for (int tid = 0; tid < temx::CLIM_THREADS; ++tid) {
              const int r = tid / s.g, j = tid - r * s.g;
              if ((tid >> 6) != ((r * s.g) >> 6)) return bad("row across waves", rows, nt, esz);
              if (r < nr && j == 0) ++owned.at((size_t)(r0 + r));
            }
          }
        } else {
          if (s.rpb != temx::CLIM_LONG_ROWS) return bad("rows per workgroup", rows, nt, esz);
          for (int64_t b = 0; b < s.nblk; ++b)
            for (int w = 0; w < temx::CLIM_LONG_ROWS; ++w) {
              const int64_t row = b * temx::CLIM_LONG_ROWS + w;
              if (row < rows) ++owned.at((size_t)row);
            }
        }
        for (int c : owned)
          if (c != 1) return bad("row not owned exactly once", rows, nt, esz);
      }
  }
  std::printf("switch_f64=%" PRId64 " switch_f32=%" PRId64 " cases=%lld\n", temx::clim_switch_nt(8), temx::clim_switch_nt(4), cases);
  return 0;
}
