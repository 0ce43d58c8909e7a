// bin_tables_main.cpp -- runs pytemdiags_amd/csrc/bin_tables.hpp (the host tables of the latitude-bin sweeps) on arrays
// from a file, for tests/test_bin_tables_host.py (which builds it plain and with AddressSanitizer + UBSan).
//   bin_tables <command> <in> <out> [numbers ...]
// <in>: raw little-endian doubles ("-": none).  <out>: records {int32 name length, name, int32 kind (0 int32, 1
// float64), int64 count, data}, the format of host_tables_main.cpp.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../pytemdiags_amd/csrc/bin_tables.hpp"

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

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: bin_tables <command> <in> <out> [numbers ...]\n");
    return 2;
  }
  const std::string cmd = argv[1];
  const std::vector<double> in = read_doubles(argv[2]);
  g_out = fopen(argv[3], "wb");
  if (!g_out) return 2;
  std::vector<double> a;
  for (int i = 4; i < argc; ++i) a.push_back(atof(argv[i]));
  if (cmd == "rows" && a.size() >= 1) {            // <in: lat [deg]> B
    BinRows br;
    const bool ok = build_bin_rows(in.data(), (int64_t)in.size(), (int)a[0], br);
    put("ok", std::vector<int>{ok ? 1 : 0, BIN_ROWS});
    if (ok) {
      put("rows", br.rows);
      put("s", br.s);
      put("chunk", br.chunk);
      put("bin_chunk0", br.bin_chunk0);
    }
  } else if (cmd == "degree") {                    // pairs of L B
    std::vector<int> J;
    std::vector<double> bound;
    for (size_t i = 0; i + 2 <= a.size(); i += 2) {
      J.push_back(bin_degree((int)a[i], (int)a[i + 1]));
      for (int j = 8; j <= BIN_MAX_DEGREE; j += 2) bound.push_back(bin_bound((int)a[i], (int)a[i + 1], j));
      J.push_back(bin_count_ok((int)a[i + 1]) ? 1 : 0);
    }
    put("J", J);
    put("bound", bound);
  } else if (cmd == "basis" && a.size() >= 2) {    // <in: lat [deg]> L B: the interpolated rows [n][L + 1]
    const int L = (int)a[0], B = (int)a[1], K = L + 1, KP = (K + 15) / 16 * 16, J = bin_degree(L, B);
    put("J", std::vector<int>{J, KP});
    if (J) {
      const std::vector<double> tab = bin_coefficients(L, B, J, KP);
      std::vector<double> Y(in.size() * (size_t)K);
      for (size_t i = 0; i < in.size(); ++i) {
        const double phi = in[i] * (M_PI / 180.0);
        const int b = bin_index(phi, B);
        bin_row(tab, J, KP, K, b, bin_local(phi, B, b), &Y[i * (size_t)K]);
      }
      put("Y", Y);
      put("a", tab);
    }
  } else {
    fprintf(stderr, "unknown command %s\n", cmd.c_str());
    return 2;
  }
  return fclose(g_out) == 0 ? 0 : 2;
}
