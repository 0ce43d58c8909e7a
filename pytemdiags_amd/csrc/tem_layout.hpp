// tem_layout.hpp -- host: what temx_plan_set_tem decides.  Which form of the latitude-class sweeps runs, how every
// launch of the TEM configuration is cut and how large every buffer of it is, as pure functions of the plan's
// dimensions, the options and what the allocator has granted so far.  The caller (temx.hip) only reads the environment,
// allocates and uploads.  No HIP, no getenv.
#ifndef TEMX_TEM_LAYOUT_HPP
#define TEMX_TEM_LAYOUT_HPP
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/temx.h"
#include "launch_shapes.hpp"
#include "shared_defs.hpp"

// build-time tunables of the latitude-class sweeps that enter a cut (the ring depths stay with the launchers)
#ifndef TEMX_CLS_E_WPS
#define TEMX_CLS_E_WPS 3
#endif
#ifndef TEMX_CLS_OP_WPS
#define TEMX_CLS_OP_WPS 1
#endif
#ifndef TEMX_CLS_MINCHUNK
#define TEMX_CLS_MINCHUNK 1
#endif

namespace temx {

// ---- waves per SIMD of the sweeps whose cut depends on them ---------------------------------------------------------
// sweep-1 configurations (temx.hip, ProjCfgC / E / 1 / 3): quads of d-tiles; small ragged D, one d-tile per workgroup;
// the single-field operator API; the 3 eddy products of the large-L path
constexpr int PROJ_C_WPS = 2, PROJ_E_WPS = 3, PROJ_1_WPS = 2, PROJ_3_WPS = 2;
constexpr int SYM_PROJ_E_WPS = 3;
constexpr int CLS_PROJ_E_WPS = TEMX_CLS_E_WPS;   // class sweep, one field per wave

// d-tiles per workgroup that waste the fewest wave slots on a ragged last workgroup
inline int pick_dpw(int ndt, int maxdpw) {
  int best = maxdpw;
  double bw = 1e9;
  for (int d = maxdpw; d >= 1; d >>= 1) {
    const double w = (double)(((ndt + d - 1) / d) * d) / ndt;
    if (w < bw - 0.05) {
      bw = w;
      best = d;
    }
  }
  return best;
}
inline int proj_dpw(int NF, int ndt) {
  if (NF == 1) return 4;
  return pick_dpw(ndt, 4) == 1 ? 1 : 4;     // small ragged D: config E (1 field per wave)
}
inline int proj_wps(int NF, int dpw) {
  if (NF == 1) return PROJ_1_WPS;
  return dpw == 1 ? PROJ_E_WPS : PROJ_C_WPS;
}

// ---- path selection: temx_plan_configure sets the options, the TEMX_* environment variables override them ----------
struct FormChoice {
  bool two_pass;      // the class path in its two-pass form
  bool force_op;      // the one-pass form wherever it is possible (lifts the size threshold)
  int os;             // single sweep: 0 never, 1 wherever the instantiations exist, -1 automatic
};
// env_*: the values of TEMX_TWO_PASS, TEMX_ONE_PASS and TEMX_SINGLE_SWEEP, null when unset
inline FormChoice form_choice(int opt_form, bool bin, const char* env_two_pass, const char* env_one_pass,
                              const char* env_single_sweep) {
  FormChoice c{false, false, -1};
  if (bin) return FormChoice{true, false, 0};   // the binned form ignores the overrides; what runs next to it
                                                // (eddies, tracers) is the plan's two-pass form
  switch (opt_form) {
    case TEMX_FORM_TWO_PASS: c.two_pass = true; c.os = 0; break;
    case TEMX_FORM_CLASS_SUMS: c.force_op = true; c.os = 0; break;
    case TEMX_FORM_SINGLE_SWEEP: c.force_op = true; c.os = 1; break;
    case TEMX_FORM_NO_SINGLE_SWEEP: c.os = 0; break;
    default: break;
  }
  if (const char* e = env_two_pass) c.two_pass = e[0] == '1';
  if (const char* e = env_one_pass) c.force_op = c.force_op || e[0] == '1';
  if (const char* e = env_single_sweep) c.os = e[0] == '0' ? 0 : (e[0] == '1' ? 1 : c.os);
  return c;
}

// the single sweep has instantiations for this plan (has_rows: the host copy of the row table is there)
inline bool os_supported(bool cls, bool large, bool weighted, bool qbasis, bool has_rows, int TBS, int L) {
  if (!cls || large || weighted || !qbasis || !has_rows) return false;
  const int tbx = (L + 1 + 3) / 4;          // blocks of 4 even harmonics up to degree 2L
  return (TBS == 7 && tbx <= 13) || (TBS == 4 && tbx <= 8) || (TBS == 2 && tbx <= 4);
}

// The memory rule of the class-sum streams: held already, or less than half of what is free (`with`: a second
// stream that has to fit next to it, the large-L path's pbuf)
inline bool fits(size_t need, size_t held, size_t free, size_t with = 0) { return held >= need || need + with < free / 2; }

// ---- the plan's dimensions, as the stages below read them ------------------------------------------------------------
struct TemDims {
  int64_t N = 0, nchunk = 0;
  int K = 0, K4 = 0, M = 0, num_cu = 0, nlev = 0;
  int64_t nt = 0;
  bool unfused_stage2 = false, lcls = false, cls = false, sym = false;
  int64_t cgroups = 0, cbatches = 0, npg = 0;
  int64_t D() const { return (int64_t)nlev * nt; }
  int ndt() const { return (int)((D() + 15) / 16); }
  // eddy sweep: one 8-wave workgroup per CU (LDS slabs) owning edpw d-tiles; the 8/edpw waves on a d-tile split its
  // chunk range -> 8/edpw partial slabs per split
  int edpw() const { return pick_dpw(ndt(), 4); }
  int64_t cunits() const { return std::max<int64_t>(1, cbatches / 4); }   // work units of ~4 batches (one cubed-sphere class-group)
  size_t KD8() const { return (size_t)K * D() * 8; }                      // bytes of [K][D] doubles
};

// ---- base: the generic sweeps and what every path needs ---------------------------------------------------------------
struct BaseLayout {
  Split sp_proj4, sp_eddy, sp_proj1;
  int edpw;
  size_t B4, B3, C4, zb;
  size_t partial, partial_unfused;   // the second: 0 unless stage 2 is unfused
};
inline BaseLayout tem_base_layout(const TemDims& d) {
  BaseLayout b{};
  const int64_t D = d.D();
  const int pdpw = proj_dpw(4, d.ndt());
  b.edpw = d.edpw();
  b.sp_proj4 = choose_split(D, d.nchunk, proj_wps(4, pdpw) * d.num_cu, pdpw);
  b.sp_eddy = choose_split(D, d.nchunk / (8 / b.edpw), d.num_cu, b.edpw);
  b.sp_proj1 = choose_split(D, d.nchunk, PROJ_1_WPS * d.num_cu);
  b.partial = (size_t)std::max(b.sp_proj4.nsplit * 4, b.sp_eddy.nsplit * (8 / b.edpw) * 3) * d.KD8();
  b.B4 = (size_t)4 * d.KD8();
  b.B3 = (size_t)3 * d.KD8();
  b.C4 = (size_t)4 * d.K4 * D * 8;
  b.zb = (size_t)8 * d.M * D * 8;
  // unfused stage 2: products are projected three at a time, 64 harmonics per pass
  b.partial_unfused = d.unfused_stage2 ? (size_t)b.sp_proj1.nsplit * 3 * 64 * D * 8 : 0;
  return b;
}

// ---- large-L class path: class sums first (kernels_cls.hpp), if they fit ----------------------------------------------
struct LargeClsLayout {
  bool eligible;            // enough d-tiles and not held to the two-pass form: taken when csum and pbuf fit
  size_t csum, pbuf;        // fits(csum, held, free, pbuf)
  Split sp_cproj4, sp_cflux, sp_lflux;
  size_t Bs, partial;
};
inline LargeClsLayout tem_large_cls_layout(const TemDims& d, const FormChoice& fc) {
  LargeClsLayout l{};
  const int64_t D = d.D();
  const int ndt = d.ndt(), edpw = d.edpw();
  l.eligible = ndt >= 4 && !fc.two_pass;
  l.csum = (size_t)d.cgroups * ndt * 14 * 64 * 8;
  l.pbuf = (size_t)d.cgroups * ndt * 3 * 128 * 8;
  l.sp_cproj4 = choose_split(D, d.cunits(), TEMX_CLS_OP_WPS * d.num_cu, 4, 8);
  l.sp_cflux = choose_split(D, std::max<int64_t>(1, d.cgroups / (8 / edpw)), d.num_cu, edpw, TEMX_CLS_MINCHUNK);
  l.sp_lflux = choose_split(D, std::max<int64_t>(1, d.cgroups / 8), d.num_cu, 1, TEMX_CLS_MINCHUNK);
  l.partial = (size_t)l.sp_cflux.nsplit * 4 * 64 * D * 8;
  l.Bs = (size_t)4 * 64 * D * 8;
  return l;
}

// ---- class path, two-pass part ----------------------------------------------------------------------------------------
struct ClsLayout {
  Split sp_cproj4, sp_cproj1, sp_ceddy;
  size_t partial;
  bool want_onepass;        // the one-pass form is wanted: taken when fits(csum, held, free) and the allocation succeeds
  size_t csum;              // 8 x 512 B per class-group and d-tile: 4 {north, south} pairs per lane
};
inline ClsLayout tem_cls_layout(const TemDims& d, const FormChoice& fc) {
  ClsLayout c{};
  const int64_t D = d.D();
  const int ndt = d.ndt(), edpw = d.edpw();
  const bool quad = edpw == 4;
  c.sp_cproj4 = choose_split(D, d.cunits(), (quad ? 2 : CLS_PROJ_E_WPS) * d.num_cu, quad ? 4 : 1, TEMX_CLS_MINCHUNK);
  c.sp_cproj1 = choose_split(D, d.cunits(), CLS_PROJ_E_WPS * d.num_cu, 4, TEMX_CLS_MINCHUNK);
  c.sp_ceddy = choose_split(D, d.cunits() / (8 / edpw), d.num_cu, edpw, TEMX_CLS_MINCHUNK);
  c.partial = (size_t)std::max({c.sp_cproj4.nsplit * 4, c.sp_ceddy.nsplit * (8 / edpw) * 3, c.sp_cproj1.nsplit}) * d.KD8();
  // one-pass form: quads of d-tiles (a ragged last quad only idles a few waves).  The one-pass sweep runs one wave
  // per SIMD, which pays once there is enough work: measured break-even near 1.2e7 elements per field
  // (ne30x72x2, 7e6: 0.137 ms two-pass vs 0.156; ne30x72x4, 1.4e7: 0.223 vs 0.203; ne120x72x2, 1.1e8: 1.44 vs 1.18)
  const bool quad_op = ndt >= 4 && (fc.force_op || (double)d.N * (double)D >= 1.2e7);
  c.want_onepass = quad_op && !fc.two_pass;
  c.csum = (size_t)d.cgroups * ndt * 8 * 64 * 8;
  return c;
}

// ---- class path, one-pass part (once csum is granted) -----------------------------------------------------------------
struct OnePassLayout {
  Split sp_cproj4;          // sweep 1: quads of d-tiles, pieces of >= 8 class-groups (its cuts are group aligned)
  Split sp_cflux;
  Split sp_copw;            // TEM + one tracer in one sweep: the four waves of a workgroup share a d-tile (one workgroup per CU)
  size_t Pq, partial;
  bool want_os;             // the single sweep is wanted: taken unless build_os_tables answers TEMX_ERANK
};
// os_ok: os_supported() of the plan; min_groups_opt: TEMX_OPT_SINGLE_SWEEP_MIN_GROUPS, negative = automatic
inline OnePassLayout tem_onepass_layout(const TemDims& d, const FormChoice& fc, bool os_ok, int min_groups_opt) {
  OnePassLayout o{};
  const int64_t D = d.D();
  const int edpw = d.edpw();
  o.sp_cproj4 = choose_split(D, d.cunits(), TEMX_CLS_OP_WPS * d.num_cu, 4, 8);
  o.sp_cflux = choose_split(D, std::max<int64_t>(1, d.cgroups / (8 / edpw)), d.num_cu, edpw, TEMX_CLS_MINCHUNK);
  o.sp_copw = choose_split(D, std::max<int64_t>(1, d.cunits() / 4), d.num_cu, 1, 8);
  o.partial = (size_t)std::max(o.sp_cflux.nsplit * 3, o.sp_cproj4.nsplit * 7) * d.KD8();
  o.Pq = (size_t)3 * d.KD8();
  // Single-sweep form of temx_tem_run (no class-sum stream), the default where the one-pass path runs and the grid has
  // enough latitude classes for the reference fit.  Both forms cost in proportion to D; the class-sum form also in
  // proportion to the rows (its store stream and the flux kernel), the single sweep pays a pre-pass and a contraction
  // that do not depend on them.  Measured break-even near 600 class-groups (ne30, 760 groups: 2.49 against 2.80 ms at
  // 72 x 91, 0.86 against 0.96 at 72 x 30; round 3, with the contraction in LDS and 96 groups in the pre-pass: 2048).
  const int64_t min_groups = min_groups_opt >= 0 ? min_groups_opt : 640;
  o.want_os = fc.os != 0 && os_ok && (fc.os == 1 || d.cgroups >= min_groups);
  return o;
}

// ---- single sweep (after build_os_tables: KX, KR, NQ and the subsample's batches are known) ---------------------------
struct SweepLayout {
  Split sp_os;              // one round of workgroups: the pre-pass is all prologue and epilogue
  Split sp_os_s;            // the pre-pass stores next to nothing, so it may be cut as finely as the chip has CUs: at
                            // D = 6552 one split per column quad left it on 103 workgroups, 0.18 ms for 430 MB
  size_t Ax, Axs, osAt, osAb, rho, rho0, partial;
};
inline SweepLayout tem_sweep_layout(const TemDims& d, int KX, int KR, int NQ, int64_t sbatches) {
  SweepLayout s{};
  const int64_t D = d.D();
  s.sp_os = choose_split(D, d.cunits(), d.num_cu, 4, 8);
  s.sp_os_s = choose_split(D, std::max<int64_t>(1, sbatches / 4), d.num_cu, 4, 2);
  s.Ax = ((size_t)4 * KX + 3 * d.K) * D * 8;
  s.partial = (size_t)std::max(s.sp_os.nsplit, s.sp_os_s.nsplit) * s.Ax;
  s.Axs = s.rho = s.rho0 = (size_t)4 * KR * D * 8;
  s.osAt = s.osAb = (size_t)4 * NQ * D * 8;
  return s;
}

// ---- mirror-paired path -------------------------------------------------------------------------------------------------
struct SymLayout {
  Split sp_sproj4, sp_sproj1, sp_seddy;   // sp_sproj1 stays empty for a small ragged D
  size_t partial;
};
inline SymLayout tem_sym_layout(const TemDims& d) {
  SymLayout s{};
  const int64_t D = d.D();
  const int edpw = d.edpw();
  const int64_t nch = (d.npg + SYM_PROJ_CH - 1) / SYM_PROJ_CH;
  if (edpw == 4) {     // quads of d-tiles, all four fields per wave
    s.sp_sproj4 = choose_split(D, nch, 2 * d.num_cu, 4);
    s.sp_sproj1 = choose_split(D, nch, 2 * d.num_cu, 4);
  } else {             // small ragged D: one d-tile per workgroup, one field per wave
    s.sp_sproj4 = choose_split(D, nch, SYM_PROJ_E_WPS * d.num_cu, 1);
  }
  s.sp_seddy = choose_split(D, d.npg / (8 / edpw), d.num_cu, edpw);
  s.partial = (size_t)std::max({s.sp_sproj4.nsplit * 4, s.sp_seddy.nsplit * (8 / edpw) * 3, s.sp_sproj1.nsplit}) * d.KD8();
  return s;
}

// ---- tracer workspaces: they follow the cuts above ---------------------------------------------------------------------
struct TracerWs {
  size_t Bq, Bq2, Ct, tz, partial;
};
inline TracerWs tracer_ws_layout(const TemDims& d, const Split& sp_proj1, const Split& sp_cproj1) {
  TracerWs w{};
  const int64_t D = d.D();
  w.Bq = d.KD8();
  w.Bq2 = (size_t)2 * d.KD8();
  w.Ct = (size_t)3 * d.K4 * D * 8;
  w.tz = (size_t)3 * d.M * D * 8;
  w.partial = (size_t)std::max(sp_proj1.nsplit, sp_cproj1.nsplit) * d.KD8();
  return w;
}
// tracers in the single-sweep form, nq of them per sweep
struct TracerOsWs {
  size_t Axq;               // projections, then the pre-pass sums
  size_t osAtq, osAbq;
  size_t Bqp;               // raw sums of the q's, then of the products
  size_t rho_t;
};
inline TracerOsWs tracer_os_ws_layout(const TemDims& d, int nq, int KX, int KR, int NQ) {
  TracerOsWs w{};
  const int64_t D = d.D();
  w.Axq = (size_t)nq * (KX + 2 * d.K + KR) * D * 8;
  w.osAtq = w.osAbq = (size_t)nq * NQ * D * 8;
  w.Bqp = (size_t)nq * 3 * d.KD8();
  w.rho_t = (size_t)4 * KR * D * 8;
  return w;
}
// temx_tem_tracer_stage1: 10 slabs per split (u v theta omega | q | u v, u omega, v theta | q v, q omega)
inline size_t tem_tracer_stage1_partial(const TemDims& d, const Split& sp_copw) { return (size_t)sp_copw.nsplit * 10 * d.KD8(); }

// ---- LDS bytes of a workgroup of the three single-sweep kernels (kernels_op2.hpp) --------------------------------------
// TBS, TBX: blocks of the plan's and of the extended basis; NF, NP, NPR: fields, products, products kept in registers
// (OsKind); DF: the projection of a finished class-group is deferred (a second buffer of Y blocks)
constexpr int OS_NBR = 2;     // reference blocks
// sweep_os_kernel (loads of 4 rows x 16 columns)
constexpr size_t sweep_os_lds(int TBS, int TBX, int NF, int NP, int /*NPR*/, int DF) {
  return ((size_t)4 * (DF ? 2 : 1) * 2 * TBX * 16 + (size_t)4 * NF * 2 * OS_NBR * 64 + (size_t)4 * NP * 2 * TBS * 64) * 8;
}
// sweep_os2_kernel (fp32 inputs, two waves per SIMD)
constexpr size_t sweep_os2_lds(int TBS, int TBX, int NF, int NP, int NPR, int /*DF*/) {
  return ((size_t)2 * 2 * TBX * 16 + 16 + (size_t)4 * NF * 2 * OS_NBR * 64 + (size_t)8 * (NP - NPR) * TBS * 64 +
          (size_t)(NF + NP) * 512) * 8;
}
// sweep_osr_kernel: Y blocks x 2 | counts | reference operands | product accumulators | exchange | the flag form's two counters
constexpr size_t sweep_osr_lds(int TBS, int TBX, int NF, int NP, int NPR, int /*DF*/) {
  return ((size_t)2 * 2 * TBX * 16 + 16 + (size_t)4 * NF * 2 * OS_NBR * 64 + (size_t)4 * (NP - NPR) * 2 * TBS * 64 +
          (size_t)2 * (NF + NP) * 256 + 2) * 8;
}

}  // namespace temx

#endif
