// host_tables_main.cpp -- runs the HIP-free host headers of pytemdiags_amd/csrc on arrays from a file, for
// tests/test_host_tables.py (which builds it plain and with AddressSanitizer + UBSan).
//   host_tables <command> <in> <out> [numbers ...]
// <in>: raw little-endian doubles ("-": none).  <out>: records {int32 name length, name, int32 kind (0 int32, 1
// float64), int64 count, data}.  Integers among the inputs travel as doubles.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../pytemdiags_amd/csrc/class_tables.hpp"
#include "../../pytemdiags_amd/csrc/host_math.hpp"
#include "../../pytemdiags_amd/csrc/launch_shapes.hpp"

using namespace temx;

static FILE* g_out = nullptr;

static void put_raw(const std::string& name, int kind, const void* data, size_t count, size_t size) {
  const int32_t nl = (int32_t)name.size(), k = kind;
  const int64_t n = (int64_t)count;
  fwrite(&nl, 4, 1, g_out);
  fwrite(name.data(), 1, name.size(), g_out);
  fwrite(&k, 4, 1, g_out);
  fwrite(&n, 8, 1, g_out);
  if (count) fwrite(data, size, count, g_out);
}
static void put(const std::string& name, const std::vector<int>& v) { put_raw(name, 0, v.data(), v.size(), 4); }
static void put(const std::string& name, const std::vector<double>& v) { put_raw(name, 1, v.data(), v.size(), 8); }
static void put(const std::string& name, const std::vector<long double>& v) { put(name, std::vector<double>(v.begin(), v.end())); }

static std::vector<double> read_doubles(const char* path) {
  std::vector<double> v;
  if (!strcmp(path, "-")) return v;
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  v.resize((size_t)ftell(f) / 8);
  fseek(f, 0, SEEK_SET);
  if (!v.empty() && fread(v.data(), 8, v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}

static void put_sides(const std::string& pre, const std::vector<int>& crow, const std::vector<int>& gbatch0, int64_t ngroups) {
  SideTables st;
  build_side_tables(crow, gbatch0, ngroups, st);
  for (int sd = 0; sd < 2; ++sd) {
    put(pre + "side" + std::to_string(sd) + "_crow", st.crow[sd]);
    put(pre + "side" + std::to_string(sd) + "_gfirst", st.gfirst[sd]);
  }
}

// classes <in: lat> <out> tol side_cap side_keep keep L nstripes nsub ...
static void cmd_classes(const std::vector<double>& lat, const std::vector<double>& a) {
  ClassTables ct;
  const bool ok = build_classes(lat.data(), (int64_t)lat.size(), ct, a[0], (size_t)a[1], (size_t)a[2]);
  put("ok", std::vector<int>{ok ? 1 : 0});
  if (!ok) return;
  put("dims", std::vector<int>{(int)ct.ncls, (int)ct.ngroups, (int)ct.nbatch, (int)ct.max_side});
  put("crow", ct.crow);
  put("xc", ct.xc);
  put("gbatch0", ct.gbatch0);
  put("cnt", ct.cnt);
  put_sides("", ct.crow, ct.gbatch0, ct.ngroups);
  const ClassSubsample ss = class_subsample(ct.crow, ct.xc, ct.gbatch0, ct.ngroups, (int64_t)a[3]);
  put("sub_dims", std::vector<int>{(int)ss.S, (int)ss.ngroups, (int)ss.nbatch});
  put("sub_crow", ss.crow);
  put("sub_xc", ss.xc);
  put("sub_gbatch0", ss.gbatch0);
  put_sides("sub_", ss.crow, ss.gbatch0, ss.ngroups);
  for (size_t i = 6; i < a.size(); ++i) {
    const int nsub = (int)a[i];
    put("cut_aligned_" + std::to_string(nsub), work_cuts(ct.gbatch0, ct.ngroups, ct.nbatch, nsub, true));
    put("cut_plain_" + std::to_string(nsub), work_cuts(ct.gbatch0, ct.ngroups, ct.nbatch, nsub, false));
    put("sub_cut_aligned_" + std::to_string(nsub), work_cuts(ss.gbatch0, ss.ngroups, ss.nbatch, nsub, true));
  }
  const int L = (int)a[4];
  if (L > 0) {
    const int K = L + 1, KX = 2 * L + 1;
    put("Gs", subsample_gram(ct.xc, ct.cnt, ct.ngroups, ss.S, std::min(16, K)));
    put("Gx", extended_gram(ct.xc, ct.cnt, ct.ncls, K, KX, (int)a[5]));
  }
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: host_tables <command> <in> <out> [numbers ...]\n");
    return 2;
  }
  const std::string cmd = argv[1];
  const std::vector<double> in = read_doubles(argv[2]);
  g_out = fopen(argv[3], "wb");
  if (!g_out) return 2;
  std::vector<double> a;
  for (int i = 4; i < argc; ++i) a.push_back(atof(argv[i]));
  auto need = [&](size_t n) {
    if (a.size() < n) {
      fprintf(stderr, "%s: %zu numbers expected\n", cmd.c_str(), n);
      exit(2);
    }
  };
  if (cmd == "classes") {
    need(6);
    cmd_classes(in, a);
  } else if (cmd == "mirror") {            // <in: lat> tol
    need(1);
    std::vector<int> rn, rs;
    const bool ok = find_mirror_pairs(in.data(), (int64_t)in.size(), rn, rs, a[0]);
    put("ok", std::vector<int>{ok ? 1 : 0});
    if (ok) put("rowN", rn), put("rowS", rs);
  } else if (cmd == "quad") {              // nq n
    need(2);
    std::vector<long double> x, w;
    gauss_legendre((int)a[0], x, w);
    put("x", x);
    put("w", w);
    const QuadBasis qb = quadrature_basis((int)a[0], (int)a[1]);
    put("Y", qb.Y);
    put("w2", qb.w2);
  } else if (cmd == "gradient") {          // <in: x>
    std::vector<double> tab;
    gradient_table(in, tab);
    put("tab", tab);
  } else if (cmd == "spd" || cmd == "pinv") {   // <in: G [K][K]> K
    need(1);
    const int K = (int)a[0];
    if (in.size() != (size_t)K * K) return 2;
    std::vector<double> Gi((size_t)K * K, 0.0);
    int rc, rank = -1;
    if (cmd == "spd") {
      std::vector<long double> Li;
      rc = spd_factor(in.data(), K, Li);
      if (rc == 0) inverse_from_factor(Li, K, Gi.data());
    } else {
      rc = sym_pinv(in.data(), K, Gi.data(), &rank);
    }
    put("rc", std::vector<int>{rc, rank});
    put("Ginv", Gi);
  } else if (cmd == "blocks4") {           // <in: A [R][K]> R K TB
    need(3);
    if (in.size() != (size_t)a[0] * (size_t)a[1]) return 2;
    put("blk", pack_blocks4(in.data(), (int)a[0], (int)a[1], (int)a[2]));
  } else if (cmd == "blocks16") {          // <in: A [.][ld]> R C ld transpose nrb4 nkb
    need(6);
    std::vector<double> blk(3, -1.0);      // appended behind what is there
    append_blocks16(blk, in.data(), (int)a[0], (int)a[1], (int)a[2], a[3] != 0.0, (int)a[4], (int)a[5]);
    put("blk", blk);
  } else if (cmd == "split") {             // <in: rows of D nchunk slots dpw minchunk>
    std::vector<int> o;
    for (size_t i = 0; i + 5 <= in.size(); i += 5) {
      const Split s = choose_split((int64_t)in[i], (int64_t)in[i + 1], (int)in[i + 2], (int)in[i + 3], (int)in[i + 4]);
      o.insert(o.end(), {s.ndt, s.nsplit, s.grid, s.dpw});
    }
    put("split", o);
  } else if (cmd == "vert") {              // <in: rows of nf nlev nt nplev tsz psz>
    std::vector<int> o;
    for (size_t i = 0; i + 6 <= in.size(); i += 6) {
      VertSlab sh{};
      size_t lds = 0;
      const bool ok = vert_slab_shape((int)in[i], (int)in[i + 1], (int64_t)in[i + 2], (int)in[i + 3], (size_t)in[i + 4], (size_t)in[i + 5], &sh, &lds);
      if (ok) o.insert(o.end(), {1, sh.cw, sh.nseg, sh.seg, sh.in_stride, sh.out_stride, sh.in_img, sh.out_img, sh.p_img, (int)lds});
      else o.insert(o.end(), 10, 0);
    }
    put("vert", o);
  } else if (cmd == "layout") {            // <in: rows of ncol nlev ntb dsz>
    std::vector<int> o;
    for (size_t i = 0; i + 4 <= in.size(); i += 4) {
      const LayoutTile t = layout_tile((int64_t)in[i], (int)in[i + 1], (int64_t)in[i + 2], (size_t)in[i + 3]);
      o.insert(o.end(), {t.tc_shift, t.kl, t.tt, t.stride, t.nct, t.nlt, t.ntt});
    }
    put("layout", o);
  } else if (cmd == "tem") {               // <in: p [nlev], lat [M]> nlev nt p0
    need(3);
    const size_t nlev = (size_t)a[0];
    if (in.size() < nlev + 2) return 2;
    const TemTables tt = tem_tables(std::vector<double>(in.begin(), in.begin() + nlev), (int64_t)a[1], a[2],
                                    std::vector<double>(in.begin() + nlev, in.end()));
    put("pg", tt.pg);
    put("lg", tt.lg);
    put("coslat", tt.coslat);
    put("fcor", tt.fcor);
    put("colscale", tt.colscale);
  } else if (cmd == "miss") {              // <in: G2, T, Gi [K][K] each, x [N]> K L
    need(2);
    const size_t K = (size_t)a[0];
    if (in.size() < 3 * K * K + 1) return 2;
    put("mtab", miss_tables(in.data(), in.data() + K * K, in.data() + 2 * K * K, in.data() + 3 * K * K,
                            (int64_t)(in.size() - 3 * K * K), (int)K, (int)a[1]));
  } else {
    fprintf(stderr, "unknown command %s\n", cmd.c_str());
    return 2;
  }
  return fclose(g_out) == 0 ? 0 : 2;
}
