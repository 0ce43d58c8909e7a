// tem_layout_main.cpp -- runs pytemdiags_amd/csrc/tem_layout.hpp on cases from a file, for
// tests/test_tem_layout_host.py (which builds it plain and with AddressSanitizer + UBSan).
//   tem_layout plan <in>    one case per line, "key=value ..." (the keys of tests/golden/tem_layouts.json); per case one line
//                           with what temx_plan_set_tem would do, given what the allocator granted: the cuts it assigns
//                           (sp_*), the bytes it asks every buffer to hold (need_*), every request to `partial` and the forms
//   tem_layout form <in>    opt_form, bin and the three environment values per line -> the FormChoice
//   tem_layout lds          the LDS bytes of the three single-sweep kernels for every (TBS, TBX) pair and kind
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

#include "../../pytemdiags_amd/csrc/tem_layout.hpp"

using namespace temx;

typedef std::map<std::string, std::string> Case;

static Case parse(const std::string& line) {
  Case c;
  std::istringstream is(line);
  std::string tok;
  while (is >> tok) {
    const size_t eq = tok.find('=');
    if (eq != std::string::npos) c[tok.substr(0, eq)] = tok.substr(eq + 1);
  }
  return c;
}
static long long num(const Case& c, const char* key) {
  const auto it = c.find(key);
  if (it == c.end()) {
    fprintf(stderr, "missing key %s\n", key);
    exit(2);
  }
  return strtoll(it->second.c_str(), nullptr, 10);
}
// an environment value as the fixture holds it: its first character, "-" when unset
static const char* env(const Case& c, const char* key) {
  const auto it = c.find(key);
  return it == c.end() || it->second == "-" ? nullptr : it->second.c_str();
}
static FormChoice form_of(const Case& c) {
  return form_choice((int)num(c, "opt_form"), num(c, "bin") != 0, env(c, "env_two_pass"), env(c, "env_one_pass"),
                     env(c, "env_single_sweep"));
}

static void put(const char* name, const Split& s) { printf(" sp_%s=%d,%d,%d,%d", name, s.ndt, s.nsplit, s.grid, s.dpw); }
static void need(const char* name, size_t bytes) { printf(" need_%s=%zu", name, bytes); }

// temx_plan_set_tem without a device: every allocation the memory rule lets through succeeds
static void plan(const Case& c) {
  TemDims d;
  d.N = num(c, "N"); d.nchunk = num(c, "nchunk"); d.K = (int)num(c, "K"); d.K4 = (int)num(c, "K4"); d.M = (int)num(c, "M");
  d.num_cu = (int)num(c, "num_cu"); d.nlev = (int)num(c, "nlev"); d.nt = num(c, "nt");
  d.unfused_stage2 = num(c, "unfused") != 0; d.lcls = num(c, "lcls") != 0; d.cls = num(c, "cls") != 0; d.sym = num(c, "sym") != 0;
  d.cgroups = num(c, "cgroups"); d.cbatches = num(c, "cbatches"); d.npg = num(c, "npg");
  const size_t held = (size_t)num(c, "b_csum"), free = (size_t)num(c, "free");
  const FormChoice fc = form_of(c);
  std::string partial;
  auto ask = [&](size_t bytes) { partial += (partial.empty() ? "" : ",") + std::to_string(bytes); };
  bool lone = false, onepass = false, os_on = false, want_onepass = false, want_os = false;
  Split cproj1;      // stays empty off the class path, as in a fresh plan

  const BaseLayout b = tem_base_layout(d);
  put("proj4", b.sp_proj4); put("eddy", b.sp_eddy); put("proj1", b.sp_proj1);
  need("B4", b.B4); need("B3", b.B3); need("C4", b.C4); need("zb", b.zb);
  ask(b.partial);
  ask(b.partial_unfused);
  if (d.lcls) {
    const LargeClsLayout l = tem_large_cls_layout(d, fc);
    if (l.eligible && fits(l.csum, held, free, l.pbuf)) {
      lone = true;
      put("cproj4", l.sp_cproj4); put("cflux", l.sp_cflux); put("lflux", l.sp_lflux);
      need("csum", l.csum); need("pbuf", l.pbuf); need("Bs", l.Bs);
      ask(l.partial);
    }
  }
  if (d.cls) {
    const ClsLayout k = tem_cls_layout(d, fc);
    Split cproj4 = k.sp_cproj4;
    ask(k.partial);
    want_onepass = k.want_onepass;
    if (k.want_onepass && fits(k.csum, held, free)) {
      onepass = true;
      const bool os_ok = os_supported(d.cls, num(c, "large") != 0, num(c, "weighted") != 0, num(c, "qbasis") != 0,
                                      num(c, "has_crow") != 0, (int)num(c, "TBS"), (int)num(c, "L"));
      const OnePassLayout o = tem_onepass_layout(d, fc, os_ok, (int)num(c, "min_groups"));
      cproj4 = o.sp_cproj4;
      put("cflux", o.sp_cflux); put("copw", o.sp_copw);
      need("csum", k.csum); need("Pq", o.Pq);
      ask(o.partial);
      want_os = o.want_os;
      if (o.want_os && num(c, "os_rc") == 0) {        // build_os_tables succeeded (TEMX_ERANK: the class-sum form stays)
        os_on = true;
        const SweepLayout s = tem_sweep_layout(d, (int)num(c, "KX"), (int)num(c, "KR"), (int)num(c, "NQ"), num(c, "sbatches"));
        put("os", s.sp_os); put("os_s", s.sp_os_s);
        need("Ax", s.Ax); need("Axs", s.Axs); need("osAt", s.osAt); need("osAb", s.osAb); need("rho", s.rho); need("rho0", s.rho0);
        ask(s.partial);
      }
    }
    put("cproj4", cproj4); put("cproj1", k.sp_cproj1); put("ceddy", k.sp_ceddy);
    cproj1 = k.sp_cproj1;
  }
  if (d.sym) {
    const SymLayout s = tem_sym_layout(d);
    put("sproj4", s.sp_sproj4); put("sproj1", s.sp_sproj1); put("seddy", s.sp_seddy);
    ask(s.partial);
  }
  // the tracer workspaces follow the cuts
  const TracerWs w = tracer_ws_layout(d, b.sp_proj1, cproj1);
  printf(" edpw=%d lone=%d onepass=%d os_on=%d want_onepass=%d want_os=%d partial_asks=%s tracer_Bq=%zu tracer_partial=%zu\n", b.edpw,
         (int)lone, (int)onepass, (int)os_on, (int)want_onepass, (int)want_os, partial.c_str(), w.Bq, w.partial);
}

static void form(const Case& c) {
  const FormChoice f = form_of(c);
  printf("two_pass=%d force_op=%d os=%d\n", (int)f.two_pass, (int)f.force_op, f.os);
}

static void lds() {
  const int pairs[3][2] = {{7, 13}, {4, 8}, {2, 4}};                 // dispatch.hpp, OsPairs
  const int kinds[3][4] = {{0, 4, 3, 0}, {1, 3, 2, 0}, {3, 4, 4, 2}};  // kernels_op2.hpp, OsKind: KIND, NF, NP, NPR
  for (const auto& p : pairs)
    for (const auto& k : kinds)
      for (int df = 0; df < 2; ++df)
        printf("TBS=%d TBX=%d kind=%d DF=%d os=%zu os2=%zu osr=%zu\n", p[0], p[1], k[0], df,
               sweep_os_lds(p[0], p[1], k[1], k[2], k[3], df), sweep_os2_lds(p[0], p[1], k[1], k[2], k[3], df),
               sweep_osr_lds(p[0], p[1], k[1], k[2], k[3], df));
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "lds")) {
    lds();
    return 0;
  }
  if (argc < 3 || (strcmp(argv[1], "plan") && strcmp(argv[1], "form"))) {
    fprintf(stderr, "usage: tem_layout plan|form <in> | lds\n");
    return 2;
  }
  std::ifstream in(argv[2]);
  if (!in) {
    fprintf(stderr, "cannot open %s\n", argv[2]);
    return 2;
  }
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    if (!strcmp(argv[1], "plan")) plan(parse(line));
    else form(parse(line));
  }
  return 0;
}
