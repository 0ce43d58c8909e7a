// tfilt_shapes_main.cpp -- pytemdiags_amd/csrc/tfilt_shapes.hpp on its own (no HIP), built with the host compiler under
// AddressSanitizer + UBSan by tests/test_tfilt_host.py.
//   cut       over a sweep of (rows, nt, nw, element sizes) the index arithmetic of kernels_tfilt.hpp is replayed lane by
//             lane: every (row, output time) is stored exactly once, every source read lies inside its row, every LDS read
//             inside the staged image, every LDS element an output that is stored depends on has been staged, the image
//             fits its budget, rpb is a power of two, TT a multiple of R, the stride odd, and no grid dimension overflows.
//   checker   every TEMX_EINVAL case of tfilt_check_args on made-up addresses, and the launch limit.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pytemdiags_amd/csrc/tfilt_shapes.hpp"

using namespace temx;

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      ++failures;                                \
      std::printf("FAILED %s: ", #cond);         \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
    }                                            \
  } while (0)

// one field, replayed as the kernel runs it
static void replay(int64_t rows, int64_t nt, int nw, size_t esz) {
  const TfiltShape sh = tfilt_shape(rows, nt, nw, 1, esz, 8);
  const int64_t nto = nt - nw + 1;
  const int R = sh.R;
  CHECK(sh.rpb >= 1 && sh.rpb <= TFILT_THREADS && (sh.rpb & (sh.rpb - 1)) == 0, "rpb %d", sh.rpb);
  CHECK(R == TFILT_R && sh.TT >= R && sh.TT % R == 0, "TT %d", sh.TT);
  CHECK(sh.stride % 2 == 1 && sh.stride >= sh.TT + nw - 1, "stride %d TT %d nw %d", sh.stride, sh.TT, nw);
  CHECK(tfilt_lds_bytes(sh, esz) <= (size_t)TFILT_LDS_BYTES, "lds %zu", tfilt_lds_bytes(sh, esz));
  CHECK(sh.ntile == (nto + sh.TT - 1) / sh.TT && sh.grid == (int64_t)sh.ntile * ((rows + sh.rpb - 1) / sh.rpb), "grid");
  CHECK(sh.grid < TFILT_GRID_MAX, "grid %lld", (long long)sh.grid);
  if (failures) return;
  std::vector<unsigned char> stored((size_t)(rows * nto), 0);
  const size_t image = (size_t)sh.rpb * sh.stride;
  std::vector<unsigned char> staged(image);
  for (int64_t g = 0; g < sh.grid; ++g) {
    const int64_t rb = g / sh.ntile;
    const int tile = (int)(g - rb * sh.ntile);
    const int64_t r0 = rb * sh.rpb;
    CHECK(r0 < rows, "workgroup %lld has no rows", (long long)g);
    const int nr = (int)(rows - r0 < sh.rpb ? rows - r0 : sh.rpb);
    const int64_t t0 = (int64_t)tile * sh.TT;
    const int tw = (int)(nto - t0 < sh.TT ? nto - t0 : sh.TT);
    const int span = tw + nw - 1;
    CHECK(tw >= 1 && t0 + span <= nt, "tile %d reads beyond its row", tile);
    staged.assign(image, 0);
    for (int tid = 0; tid < TFILT_THREADS; ++tid) {   // load side
      const int lane = tid & 63, wv = tid >> 6;
      for (int rbase = wv; rbase < nr; rbase += 4 * 4)
        for (int e = lane; e < span; e += 64)
          for (int q = 0; q < 4; ++q) {
            const int r = rbase + 4 * q;
            if (r >= nr) continue;
            const int64_t src = (r0 + r) * nt + t0 + e;
            CHECK(src >= 0 && src < rows * nt && src / nt == r0 + r, "source read outside its row");
            const size_t a = (size_t)r * sh.stride + e;
            CHECK(a < image && !staged[a], "LDS element staged twice or outside the image");
            if (a < image) staged[a] = 1;
          }
    }
    for (int tid = 0; tid < TFILT_THREADS; ++tid) {   // filter side
      const int r = tid & (sh.rpb - 1);
      if (r >= nr) continue;
      const int rl = tid / sh.rpb, step = (TFILT_THREADS / sh.rpb) * R;
      for (int j0 = rl * R; j0 < tw; j0 += step) {
        const size_t p = (size_t)r * sh.stride + j0;
        // the run reads p[0 .. R + nw - 1): the first window, then a refill p[k + R] at every k with k + 1 < nw
        CHECK(p + R + nw - 2 < (size_t)(r + 1) * sh.stride && p + R + nw - 2 < image, "LDS read outside the row's stride");
        for (int j = 0; j < R; ++j) {
          if (j0 + j >= tw) continue;
          // (a row is staged as one piece, [0, span): the two ends of the window stand for it)
          CHECK(staged[p + j] && staged[p + j + nw - 1], "a stored output reads an element that was not staged");
          const int64_t o = (r0 + r) * nto + t0 + j0 + j;
          CHECK(o >= 0 && o < rows * nto && !stored[(size_t)o], "output stored twice or outside the destination");
          if (o >= 0 && o < rows * nto) stored[(size_t)o] = 1;
        }
      }
    }
    if (failures) return;
  }
  for (int64_t i = 0; i < rows * nto; ++i)
    if (!stored[(size_t)i]) {
      CHECK(false, "output %lld of rows %lld nt %lld nw %d esz %zu was never stored", (long long)i, (long long)rows, (long long)nt, nw, esz);
      return;
    }
}

int main() {
  // ---- the cut ----
  int shapes = 0;
  const int nws[] = {1, 3, 9, 31, 95, 97, 121, 191, 193, 255};
  const int64_t rowss[] = {1, 7, 31, 33, 255, 257, 1000};
  for (size_t esz : {(size_t)8, (size_t)4})
    for (int nw : nws)
      for (int64_t rows : rowss) {
        const TfiltShape s0 = tfilt_shape(rows, nw + 4000, nw, 1, esz, 8);
        const int64_t ntos[] = {1, 2, 7, 8, 9, 63, 64, 65, 100, 129, s0.TT, s0.TT + 3, 2 * s0.TT + 1, 610};
        for (int64_t nto : ntos) {
          if (rows * nto > 60000) continue;   // (the replay is per output)
          replay(rows, nto + nw - 1, nw, esz);
          ++shapes;
          if (failures) {
            std::printf("at rows %lld nto %lld nw %d esz %zu\n", (long long)rows, (long long)nto, nw, esz);
            return 1;
          }
        }
      }
  // the cut does not depend on the number of rows, the bands or the destination (only the grid does)
  for (int nw : nws) {
    const TfiltShape a = tfilt_shape(5, 730, nw, 1, 8, 8), b = tfilt_shape(3499344, 730, nw, 4, 8, 8);
    CHECK(a.rpb == b.rpb && a.TT == b.TT && a.stride == b.stride && a.ntile == b.ntile, "cut depends on rows or nb");
  }
  // the shapes of the measurements: 32 rows per workgroup unless the halo leaves no room
  CHECK(tfilt_shape(3499344, 730, 31, 1, 8, 8).rpb == 32 && tfilt_shape(3499344, 730, 31, 1, 8, 8).TT == 128, "ne30 fp64 nw 31");
  CHECK(tfilt_shape(3499344, 730, 121, 1, 8, 8).rpb == 16 && tfilt_shape(3499344, 730, 121, 1, 8, 8).TT == 128, "ne30 fp64 nw 121");
  CHECK(tfilt_shape(3499344, 730, 255, 1, 8, 8).rpb == 8 && tfilt_shape(3499344, 730, 255, 1, 8, 8).TT == 256, "ne30 fp64 nw 255");
  CHECK(tfilt_shape(3499344, 730, 121, 1, 4, 4).rpb == 32 && tfilt_shape(3499344, 730, 121, 1, 4, 4).TT == 192, "ne30 fp32 nw 121");
  CHECK(tfilt_shape(55987344, 120, 31, 2, 4, 4).rpb == 32 && tfilt_shape(55987344, 120, 31, 2, 4, 4).ntile == 1, "ne120 fp32 nw 31");
  CHECK(tfilt_shape(1000, 3, 3, 1, 8, 8).rpb == 256, "a record of one output: 256 rows per workgroup");
  // ---- the launch limit ----
  CHECK(tfilt_shape((int64_t(1) << 29) - 32, 80, 9, 1, 8, 8).grid < TFILT_GRID_MAX, "just below the limit");
  CHECK(tfilt_shape(int64_t(1) << 29, 80, 9, 1, 8, 8).grid >= TFILT_GRID_MAX, "at the limit");

  // ---- the checker, on made-up addresses ----
  int refusals = 0;
  const int64_t ncol = 10, nt = 40;
  const int nlev = 2, nw = 9;
  const size_t src_bytes = (size_t)ncol * nlev * nt * 8, dst_bytes = (size_t)ncol * nlev * (nt - nw + 1) * 8;
  char* const base = (char*)(uintptr_t)(1 << 20);
  const void* src[2] = {base, base + src_bytes};
  const int f64[2] = {TEMX_F64, TEMX_F64}, f32[2] = {TEMX_F32, TEMX_F32}, bad[2] = {TEMX_F64, 7};
  char* const d0 = base + 2 * src_bytes;
  void* dst[4] = {d0, d0 + dst_bytes, d0 + 2 * dst_bytes, d0 + 3 * dst_bytes};
  const double* w = (const double*)(d0 + 4 * dst_bytes);
  auto ok = [&](const Refusal& r) { return r.code == TEMX_OK; };
  auto no = [&](const Refusal& r, const char* what) {
    ++refusals;
    const bool hit = r.code == TEMX_EINVAL && r.msg[0];
    if (!hit) std::printf("FAILED: %s was not refused\n", what), ++failures;
  };
  CHECK(ok(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0)), "a good call is refused");
  CHECK(ok(tfilt_check_args(2, src, f32, 2, dst, TEMX_F32, ncol, nlev, nt, nw, w, 0)), "a good fp32 call is refused");
  CHECK(ok(tfilt_check_args(2, src, f32, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0)), "a good widening call is refused");
  CHECK(ok(tfilt_check_args(1, src, f64, 1, dst, TEMX_F64, ncol, nlev, nw, nw, w, 0)), "nt = nw is refused");
  no(tfilt_check_args(0, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "nf = 0");
  no(tfilt_check_args(9, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "nf = 9");
  no(tfilt_check_args(2, nullptr, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "null src_host");
  no(tfilt_check_args(2, src, nullptr, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "null src_dtype_host");
  no(tfilt_check_args(2, src, f64, 2, nullptr, TEMX_F64, ncol, nlev, nt, nw, w, 0), "null dst_host");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, nullptr, 0), "null weights");
  no(tfilt_check_args(2, src, f64, 0, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "nb = 0");
  no(tfilt_check_args(2, src, f64, 5, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "nb = 5");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, 0, w, 0), "nw = 0");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, 400, 257, w, 0), "nw = 257");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, 8, w, 0), "nw even");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, 8, nw, w, 0), "nt < nw");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, 0, nlev, nt, nw, w, 0), "ncol = 0");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, 0, nt, nw, w, 0), "nlev = 0");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, 0, nw, w, 0), "nt = 0");
  no(tfilt_check_args(2, src, bad, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "unknown src dtype");
  no(tfilt_check_args(2, src, f64, 2, dst, 5, ncol, nlev, nt, nw, w, 0), "unknown dst dtype");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 1), "unknown flag");
  no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F32, ncol, nlev, nt, nw, w, 0), "fp64 source, fp32 destination");
  {
    const void* s2[2] = {base, nullptr};
    no(tfilt_check_args(2, s2, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "null src");
    const void* s3[2] = {base, base + src_bytes + 4};
    no(tfilt_check_args(2, s3, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0), "misaligned src");
    CHECK(ok(tfilt_check_args(2, s3, f32, 2, dst, TEMX_F64, ncol, nlev, nt, nw, w, 0)), "an fp32 source at 4 mod 8 is refused");
    void* d2[4] = {dst[0], dst[1], nullptr, dst[3]};
    no(tfilt_check_args(2, src, f64, 2, d2, TEMX_F64, ncol, nlev, nt, nw, w, 0), "null dst");
    void* d3[4] = {dst[0], dst[1], (char*)dst[2] + 4, dst[3]};
    no(tfilt_check_args(2, src, f64, 2, d3, TEMX_F64, ncol, nlev, nt, nw, w, 0), "misaligned dst");
    no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, (const double*)((const char*)w + 4), 0), "misaligned weights");
    void* d4[4] = {dst[0], dst[1], dst[2], (char*)src[1] + src_bytes - 8};
    no(tfilt_check_args(2, src, f64, 2, d4, TEMX_F64, ncol, nlev, nt, nw, w, 0), "dst overlaps src");
    void* d5[4] = {dst[0], dst[1], dst[2], (char*)dst[2] + dst_bytes - 8};
    no(tfilt_check_args(2, src, f64, 2, d5, TEMX_F64, ncol, nlev, nt, nw, w, 0), "dst overlaps dst");
    no(tfilt_check_args(2, src, f64, 2, dst, TEMX_F64, ncol, nlev, nt, nw, (const double*)((char*)dst[3] + dst_bytes - 8), 0),
       "dst overlaps weights");
    void* d6[4] = {dst[0], dst[1], dst[2], (char*)dst[2] + dst_bytes};
    CHECK(ok(tfilt_check_args(2, src, f64, 2, d6, TEMX_F64, ncol, nlev, nt, nw, w, 0)), "touching extents are refused");
  }
  std::printf("shapes=%d refusals=%d %s\n", shapes, refusals, failures ? "FAILED" : "cut=ok checker=ok");
  return failures ? 1 : 0;
}
