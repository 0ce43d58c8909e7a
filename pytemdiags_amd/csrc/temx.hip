// temx.hip -- host side of libtemx.so: plan, workspace, launch logic and the C ABI of
// include/temx.h.  gfx950 only.  Build: see csrc/Makefile (hipcc --offload-arch=gfx950).
// What can be decided without a device is not here: the tables and launch shapes of a plan, the argument rules, the
// dispatch lists, and the form, cuts and buffer sizes of the TEM configuration (tem_layout.hpp) are HIP-free headers.
#include "../../include/temx.h"
#include "../../include/temx_vert.h"
#include "../../include/temx_layout.h"
#include "../../include/temx_ingest.h"
#include "../../include/temx_clim.h"
#include "../../include/temx_mtracer.h"
#include "../../include/temx_nclim.h"
#include "../../include/temx_gclim.h"
#include "../include/temx_mgclim.h"
#include "../include/temx_wave.h"
#include "../include/temx_tfilt.h"
#include "../include_wavecls/temx_wavecls.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <atomic>
#include <vector>

#include "kernels.hpp"
#include "kernels_sym.hpp"
#include "kernels_cls.hpp"
#include "kernels_op.hpp"
#include "kernels_op2.hpp"
#include "kernels_osc.hpp"
#include "kernels_miss.hpp"
#include "kernels_mtracer.hpp"
#include "kernels_bin.hpp"
#include "kernels_vert.hpp"
#include "kernels_layout.hpp"
#include "kernels_ingest.hpp"
#include "kernels_clim.hpp"
#include "kernels_nclim.hpp"
#include "kernels_gclim.hpp"
#include "kernels_mgclim.hpp"
#include "kernels_wave.hpp"
#include "kernels_wavecls.hpp"
#include "kernels_tfilt.hpp"
// host code without HIP: the tables, matrices and launch shapes of a plan
#include "bin_tables.hpp"
#include "class_tables.hpp"
#include "clim_shapes.hpp"
#include "nclim_shapes.hpp"
#include "dispatch.hpp"
#include "field_args.hpp"
#include "gclim_tables.hpp"
#include "host_math.hpp"
#include "launch_shapes.hpp"
#include "mgclim_shapes.hpp"
#include "tem_layout.hpp"
#include "tfilt_shapes.hpp"
#include "wave_class_tables.hpp"
#include "wave_tables.hpp"

using namespace temx;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// A failed HIP call is reported through the return code and temx_last_error().  HIP also keeps it as the thread's
// last error until somebody reads it: it is read here, so that the caller's next HIP call (torch checks
// hipGetLastError() after its own launches) does not report this library's failure as its own.
#define HIPCHK(expr)                                                                     \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      (void)hipGetLastError();                                                           \
      return fail(e_ == hipErrorOutOfMemory ? TEMX_ENOMEM : TEMX_EHIP, "%s failed: %s",  \
                  #expr, hipGetErrorString(e_));                                         \
    }                                                                                    \
  } while (0)

// the argument rules of field_args.hpp: a refused call returns through fail()
#define ARGCHK(expr) \
  do { if (const Refusal r_ = (expr)) return fail(r_.code, "%s", r_.msg); } while (0)

// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int ensure(size_t need) {
    if (need <= bytes) return TEMX_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, need);
    if (e != hipSuccess) return fail(TEMX_ENOMEM, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
    bytes = need;
    return TEMX_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  double* d() const { return static_cast<double*>(p); }
};

struct TimedLaunch {
  hipEvent_t a, b;
};

struct temx_plan {
  int device = 0, num_cu = 256;
  int64_t N = 0, nchunk = 0;
  int L = 0, K = 0, TB = 0, K4 = 0, M = 0;
  // harmonics beyond one fused sweep (K > 64): slices of 16 blocks, `stride` blocks stored per group
  int stride = 0, nslice = 1;
  bool large = false;
  DevBuf Bs, XB, P3;             // large-L path: slice sums, native means [4][N][D], products [3][N][D]
  bool finalized = false;
  bool weighted = false;      // weights mode (temx_plan_set_weights): projection rows are scaled, reconstruction rows are not
  int rank = 0;               // numerical rank of Y0 (== K unless the pseudo-inverse fallback ran)
  DevBuf x, Y0, yblk, yblk_w, Y0p, G, Ginv, norm, flag;
  DevBuf gblk, ypblk;            // Ginv / Qp as 4x4 MFMA A-operand blocks (solve_mfma_kernel, K <= 64)
  // Projection basis (temx_plan_finalize): qbasis = the sweeps project on Q = Y0 R^-1, R the Cholesky factor of
  // the Gram matrix, T = R^-1 on the device.  Qp = Y0p T is the operand that takes coefficients to the output
  // latitudes (Y0p itself stays the attribute), Ginv the inverse of the second Gram matrix Q^T Q (the identity up
  // to rounding), GinvA = T T^T the inverse of the Gram matrix of Y0 (attributes Y0inv / sanity numbers only).
  bool qbasis = false;
  bool g_checker = false;      // the Gram matrix the plan was finalised with is a checkerboard (odd entries cleared)
  bool ext_G = false;          // finalised with a Gram matrix from outside (ncol-sharded: the all-reduced one)
  bool os_need_global = false; // single sweep: this rank's own subsample cannot be fitted, the job's matrices are awaited
  DevBuf T, Qp, GinvA, G2, xo, xc;
  int64_t cls_npad = 0;
  const double* yproj_ptr() const { return yblk_w.p ? yblk_w.d() : yblk.d(); }
  std::vector<double> lat_out_deg;
  // TEM configuration
  bool tem = false;
  int nlev = 0;
  int64_t nt = 0, D = 0;
  double p0 = 101325.0;
  DevBuf p, pg, lg, coslat, fcor, colscale;
  DevBuf B4, B3, C4, zb;
  DevBuf Bq, Bq2, Ct, tz;          // tracer workspace: sums, coefficients (q, v, w), zonal means
  Split sp_proj1;
  // mirror-paired path (equatorially symmetric grids), see kernels_sym.hpp
  bool sym = false;
  int TBS = 0;
  int64_t npair = 0, npg = 0, npg_alloc = 0;
  DevBuf rows, ysym;
  Split sp_sproj4, sp_sproj1, sp_seddy;
  Split sp_proj4, sp_eddy;
  // latitude-class path (columns sharing a latitude share a basis row), see kernels_cls.hpp
  bool cls = false;
  int64_t cgroups = 0, cbatches = 0, ncls = 0;
  int64_t cls_max_side = 0;            // members of the longest class side (build_classes; TEMX_F32_SIDE_CAP)
  std::vector<int> gbatch0;            // first batch of every class-group (+ total)
  DevBuf crow, ycls;
  std::map<int, DevBuf> csplits;       // work cuts per number of pieces
  Split sp_cproj4, sp_cproj1, sp_ceddy, sp_cflux;
  // single-sweep form (kernels_op2.hpp, sweep_os_kernel): no class-sum stream; see build_os_tables / tem_run_os
  bool os_built = false, os_on = false;
  bool os_valid = false;               // Ax / rho / C4 are those of the latest single-sweep temx_tem_run (its v, omega serve the tracer)
  DevBuf Axq, rho_t;                   // tracer in the single-sweep form: [KX + 2 K][D] projections (+ [KR][D] pre-pass sums), references of (q, v, omega)
  int TBX = 0, KX = 0, KR = 0, NQ = 0;
  std::vector<double> h_xc, h_cnt;     // host copies of the class latitudes (cos colat) and member counts
  std::vector<int> h_crow;             // host copy of the row table
  std::vector<int> sgbatch0;           // subsample of class-groups (reference pre-pass): first batch of each (+ total)
  int64_t sgroups = 0, sbatches = 0;
  DevBuf ycx, ycx_s, crow_s, rho, rho0, gaunt /* Yq[NQ][KX] */, wq2, Gx, Gsinv, Ax /* [4 KX + 3 K][D]: projections of the fields, then of the products */, Axs /* [4][KR][D] */;
  std::vector<double> h_G_own;         // Y0^T Y0 over this rank's rows, kept when temx_plan_finalize installs the job's matrix
  std::vector<double> h_Gx_own;        // Gx over this rank's rows, as built: what temx_get_matrix(TEMX_MAT_GX) hands out
  std::vector<double> h_Gx, h_Gs;      // this plan's rows: Y0^T Y0ext [K][KX] and the subsample's Gram matrix [KR][KR] (all-reduced when ncol-sharded)
  // contraction of the single sweep on the matrix cores (kernels_osc.hpp): host copies of its matrices, their 4x4
  // blocks on the device (one buffer), the synthesised fields At / ab [4][NQ][D] (kept: the tracer pairs with v, omega)
  std::vector<double> h_T, h_Ginv, h_G, h_Yq;
  DevBuf oscblk, osAt, osAb, osAtq, osAbq, Bqp;
  OscMats osc{};
  bool osc_lds = false;                // TEMX_OPT_OS_CONTRACT = 1 / TEMX_OS_CONTRACT=lds: the round-3 LDS form (A/B)
  int opt_os_contract = -1;
  bool os_barrier = false;             // TEMX_OPT_OS_SYNC = 1 / TEMX_OS_SYNC=barrier: the single sweep of fp64 fields hands its
  int opt_os_sync = -1;                // class sums over through two workgroup barriers per group instead of LDS flags (A/B)
  int os_keep = 32;                    // class-groups of the reference subsample (TEMX_OPT_OS_SUBSAMPLE): 128 latitudes for 16 coefficients per column
  // what the tail of the pipeline (solve, contraction, scan, epilogue) currently describes: the snapshots
  // [tt0, tt0 + tnt) of the run, tD = nlev * tnt columns.  The whole run unless a time-sliced tail ran last.
  int64_t tD = 0, tnt = 0, tt0 = 0;
  // path selection (temx_plan_configure; the TEMX_* environment variables override): -1 = automatic
  int opt_form = -1, opt_os_map = -1, opt_op_map = -1, opt_tracer_one_pass = -1, opt_single_sweep_min_groups = -1;
  bool os_tile = false, op_tile = false;   // effective lane map of the loads (fixed in temx_plan_set_tem)
  bool no_qr = false;                      // TEMX_NO_QR (flag of temx_plan_create or environment)
  DevBuf side_crow[2][2], side_gfirst[2][2];   // [full table, subsample][north, south]: side_tables.hpp (sweep_os2_kernel)
  std::map<int, DevBuf> csplits_s;
  Split sp_os, sp_os_s;
  Split sp_copw;                 // TEM + tracer in one sweep (sweep_opw_kernel<.., 2>): one d-tile per workgroup
  // one-pass form of the class path: sweep 1 also stores per-class sums of products (csum), the
  // flux kernel replaces sweep 2 (kernels_cls.hpp)
  // large-L class path (64 < K <= 256 with latitude classes): class sums first, then sliced work on the sums
  bool lcls = false, lone = false, xb_valid = false;
  DevBuf ycls_l, pbuf;
  int64_t ycls_lstride = 0;
  Split sp_lflux;
  // op_valid: csum (and Pq) hold the class sums of the latest temx_tem_stage1 on this plan
  bool onepass = false, op_valid = false;
  // c4_valid: C4 holds the coefficients of the fields of the latest temx_tem_stage1 (a stage-2 solve has run since)
  bool c4_valid = false;
  DevBuf csum, ccnt;
  DevBuf Pq;                     // [3][K][D] projections of the co-moments of u v, u omega, v theta (sweep 1)
  // one-pass tracer: class sums of q ([groups][d-tiles][64] {north, south} pairs) and the projected
  // co-moments of q v, q omega; tq_valid: they describe the latest temx_tracer_stage1_sums
  DevBuf csq, Pq2;
  bool tq_valid = false;
  // shared workspaces
  DevBuf partial;
  // operator-API workspace (any D)
  DevBuf opB, opC;
  // missing-value mode (kernels_miss.hpp; TEMX_OPT_MISSING, TEMX_OPT_MIN_COVERAGE, TEMX_OPT_MISSING_WEIGHT)
  int opt_missing = 0, opt_min_cov = 500, opt_miss_w = 10;
  bool miss_built = false;             // eblk and mtab describe the plan's current basis
  bool miss_valid = false;             // mC / mCcov hold the coefficients of the latest masked temx_tem_run
  int64_t miss_cov_D = -1;             // columns of the coverage of the latest masked run (-1: none yet)
  int NE = 0, NQM = 0;                 // raw harmonics of the missing indicator (2L+1), Gauss nodes of H (2L+1)
  DevBuf eblk;                         // raw rows to degree 2L as 4x4 blocks, 2 TB blocks per group
  DevBuf mtab;                         // G2 [K][K], Zq [NQ][K], Yq [NQ][NE], Acov [K][K], c1 [K]
  DevBuf mB, mC, mCcov, mcov, mZ;      // sums [4K + NE][D], coefficients [4][K4][D], coverage coefficients [K4][D],
                                       // coverage [M][D], zonal scratch of the native operator [M][D]
  // masked tracer run (kernels_mtracer.hpp, include/temx_mtracer.h): allocated at the first temxm_tracer_run
  bool mt_valid = false;               // mtC / mtCcov hold the tracer of a temxm_tracer_run that followed the latest masked temx_tem_run
  DevBuf mtB, mtB2, mtC, mtCcov, mtz;  // sums [K + NE][D] and [2 K][D], coefficients (q, v, omega) [3][K4][D], coverage
                                       // coefficients of the tracer's mask [K4][D], qb qpvpb qpwappb [3][M][D]
  // latitude-bin form (kernels_bin.hpp, bin_tables.hpp; TEMX_OPT_LAT_BINS): nothing here is built or allocated before the
  // first binned temx_plan_set_tem / operator call
  int opt_lat_bins = 0;                // B in effect, 0 = off
  int bin_J = 0, bin_KP = 0;           // Chebyshev terms per bin (8, 10 or 12), K rounded up to a multiple of 16
  int bin_built = 0;                   // the B the tables on the device were built for (0: none, or another basis since)
  int bin_pass = 0;                    // > 0 inside a run entry point that goes through the staged ones (temx_tracer_run)
  int64_t bin_nchunk = 0;
  std::vector<double> h_lat;           // native latitudes in degrees, as given (the bins are cut in phi, not in cos(colat))
  DevBuf bin_a, bin_chunk, bin_c0, bin_rows, bin_s;   // a[B][J][KP], chunk list [nchunk] int4, first chunk per bin [B + 1], sorted rows, their s
  DevBuf bin_T;                        // [2][KP][KP]: T^T (sums Y -> Q) and T (coefficients Q -> Y), zero padded; identities without Q
  DevBuf bin_cm, bin_z, bin_cy;        // chunk moments [nchunk][NF][J][Dpad], series [B][NF][J][Dpad], Y coefficients [NF][K][D]
  // timing hooks
  bool timing = false;
  std::vector<TimedLaunch> timed[2];
};

static int upload(DevBuf& b, const void* src, size_t bytes) {
  int rc = b.ensure(bytes);
  if (rc) return rc;
  HIPCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return TEMX_OK;
}

// A buffer that a sweep streams into while it reads the fields.  On MI355X the write bandwidth of a large
// allocation is bimodal with its physical placement -- a zero fill of 6.7 GB runs at 5.3-5.6 or at 6.3-6.5
// TB/s, reads do not care -- and a sweep whose class sums go to a slow one loses ~5 % (tools/sweep_lab.hip
// built with -DLAB_OFFSETS, profiles/r03_lab_csum_placement.log).  So: allocate up to TEMX_PLACE_TRIES
// candidates (held together, so that each comes from other memory), time a zero fill of each, keep the
// fastest.  The fill is also the initialisation the callers need.  Small buffers are not probed.
__global__ void fill_zero_kernel(double2* __restrict__ p, int64_t n) {
  const double2 z = make_double2(0.0, 0.0);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = z;
}

static int alloc_write_stream(DevBuf& b, size_t need) {
  need = (need + 15) & ~(size_t)15;
  if (b.bytes >= need) return TEMX_OK;          // (kept from an earlier configuration: already chosen)
  int tries = 4;
  if (const char* e = getenv("TEMX_PLACE_TRIES")) tries = std::max(1, std::min(8, atoi(e)));
  if (need < ((size_t)1 << 30)) tries = 1;
  b.release();
  std::vector<DevBuf> cand;
  std::vector<float> ms;
  hipEvent_t ea = nullptr, eb = nullptr;
  if (tries > 1 && (hipEventCreate(&ea) != hipSuccess || hipEventCreate(&eb) != hipSuccess)) tries = 1;
  int best = -1;
  float slowest = 0.f;
  for (int t = 0; t < tries; ++t) {
    size_t fr = 0, tot = 0;
    if (t > 0 && (hipMemGetInfo(&fr, &tot) != hipSuccess || need > fr / 2)) break;
    DevBuf c;
    if (c.ensure(need) != TEMX_OK) {
      if (t == 0) return TEMX_ENOMEM;
      break;
    }
    float best_ms = 1e30f;
    for (int rep = 0; rep < (tries > 1 ? 2 : 1); ++rep) {
      if (ea) (void)hipEventRecord(ea, nullptr);
      hipLaunchKernelGGL(fill_zero_kernel, dim3(2048), dim3(256), 0, nullptr, static_cast<double2*>(c.p), (int64_t)(need / 16));
      if (ea) {
        float m = 0.f;
        (void)hipEventRecord(eb, nullptr);
        if (hipEventSynchronize(eb) == hipSuccess && hipEventElapsedTime(&m, ea, eb) == hipSuccess) best_ms = std::min(best_ms, m);
      }
    }
    cand.push_back(c);
    ms.push_back(best_ms);
    if (best < 0 || best_ms < ms[(size_t)best]) best = t;
    slowest = std::max(slowest, best_ms);
    // stop once both modes have been seen (or the first candidate is plainly a fast one)
    if ((double)need / (best_ms * 1e-3) >= 6.1e12 || ms[(size_t)best] < 0.92f * slowest) break;
  }
  if (ea) (void)hipEventDestroy(ea);
  if (eb) (void)hipEventDestroy(eb);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipGetLastError());
  for (size_t i = 0; i < cand.size(); ++i)
    if ((int)i == best) b = cand[i]; else cand[i].release();
  return TEMX_OK;
}

// hipFuncSetAttribute is per device: remember, per kernel instantiation, which devices have the
// dynamic-LDS limit raised (a process may own plans on several GPUs).
static int lds_attr_once(std::atomic<uint64_t>& done, int device, const void* fn, int bytes) {
  const uint64_t bit = 1ull << (device & 63);
  if (done.load(std::memory_order_acquire) & bit) return TEMX_OK;
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.fetch_or(bit, std::memory_order_release);
  return TEMX_OK;
}

// One launch: raise the dynamic-LDS limit of kernel Kern on this device if nobody has yet (to attr_bytes when given,
// else to what this launch asks for), launch, read the launch error.  The flag is the kernel instantiation's own.
template <auto Kern>
static std::atomic<uint64_t> lds_attr_done{0};   // one bit per device

template <auto Kern, typename... A>
__attribute__((noinline))   // keeps each dispatch branch a call, not an inlined launch body
static int launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, A... args) {
  hipLaunchKernelGGL(Kern, grid, block, lds_bytes, st, args...);
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}
template <auto Kern, int attr_bytes = 0, typename... A>
static int launch_lds(int device, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, A... args) {
  const int limit = attr_bytes ? attr_bytes : (int)lds_bytes;
  if (int rc = lds_attr_once(lds_attr_done<Kern>, device, reinterpret_cast<const void*>(Kern), limit)) return rc;
  return launch<Kern>(grid, block, lds_bytes, st, args...);
}

// the one dtype refusal; by_dtype: f(TypeTag<double or float>) (dispatch.hpp), or that refusal
static int bad_dtype() { return fail(TEMX_EINVAL, "dtype must be TEMX_F64 or TEMX_F32"); }
template <typename F>
static int by_dtype(int dtype, F&& f) {
  int rc = TEMX_OK;
  return dispatch_dtype(dtype, rc, f) ? rc : bad_dtype();
}

// the basis kernels keep one row of K values per thread: 64 in registers, 512 (L <= 511) in scratch
template <typename F>
static int by_basis_rows(int K, F&& f) { return K <= 64 ? f(Int<64>{}) : f(Int<512>{}); }

template <typename T>
static int upload(DevBuf& b, const std::vector<T>& v) { return upload(b, v.data(), v.size() * sizeof(T)); }
static int os_upload_blocks(temx_plan* pl);

static int set_ginv(temx_plan* pl, const double* Gi_host) {
  HIPCHK(hipMemcpy(pl->Ginv.p, Gi_host, (size_t)pl->K * pl->K * 8, hipMemcpyHostToDevice));
  pl->h_Ginv.assign(Gi_host, Gi_host + (size_t)pl->K * pl->K);
  if (pl->os_built)
    if (int rc = os_upload_blocks(pl)) return rc;
  if (pl->K > 64) return TEMX_OK;
  // Ginv padded to 4*TB rows: pack_blocks4 wants TB row-blocks
  std::vector<double> Gp((size_t)4 * pl->TB * pl->K, 0.0);
  std::copy(Gi_host, Gi_host + (size_t)pl->K * pl->K, Gp.begin());
  return upload(pl->gblk, pack_blocks4(Gp.data(), 4 * pl->TB, pl->K, pl->TB));
}

constexpr size_t kMaxTimedLaunches = 256;   // enough for an average; bounds the events a long run creates

static void time_begin(temx_plan* pl, int which, hipStream_t st, TimedLaunch& tl) {
  tl.a = tl.b = nullptr;
  if (!pl->timing || pl->timed[which].size() >= kMaxTimedLaunches) return;
  (void)hipEventCreate(&tl.a);
  (void)hipEventCreate(&tl.b);
  (void)hipEventRecord(tl.a, st);
}
static void time_end(temx_plan* pl, int which, hipStream_t st, TimedLaunch& tl) {
  if (!pl->timing || tl.a == nullptr) return;
  (void)hipEventRecord(tl.b, st);
  pl->timed[which].push_back(tl);
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// sweep-1 configurations (fields per wave, X ring depth, waves per SIMD).  Measured on
// ne120x72x30: 2 fields/wave with 2- or 3-deep rings at 3 waves/SIMD were within +-3 % of this.
// (the waves per SIMD enter the cuts: tem_layout.hpp, with pick_dpw / proj_dpw / proj_wps)
struct ProjCfgC { static constexpr int NFW = 4, PD = 1, WPS = PROJ_C_WPS; };   // default: quads of d-tiles
struct ProjCfgE { static constexpr int NFW = 1, PD = 2, WPS = PROJ_E_WPS; };   // small ragged D: one d-tile per workgroup
struct ProjCfg1 { static constexpr int NFW = 1, PD = 2, WPS = PROJ_1_WPS; };   // single-field operator API / Gram
struct ProjCfg3 { static constexpr int NFW = 3, PD = 1, WPS = PROJ_3_WPS; };   // the 3 eddy products (large-L path)

template <int NF>
static int launch_project(temx_plan* pl, const FieldPtrs<NF>& fp, int dtype, int64_t D,
                          const double* colscale, int sfield, double* partial, const Split& sp,
                          hipStream_t st, int tb_off = 0, int Kloc = -1) {
  if (Kloc < 0) Kloc = pl->K;
  return by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto go = [&](auto cfg) {
      using Cfg = decltype(cfg);
      return dispatch(TBValues{}, pl->TB, [&](auto tb) {
        return launch<project_kernel<T, NF, Cfg::NFW, decltype(tb)::value, Cfg::PD, Cfg::WPS>>(
            dim3(sp.grid), dim3(256), 0, st, fp, pl->N, D, Kloc, pl->yproj_ptr(), pl->stride, tb_off, pl->nchunk, colscale,
            sfield, partial, sp.nsplit, sp.ndt);
      });
    };
    if constexpr (NF == 1) return go(ProjCfg1{});
    else if constexpr (NF == 3) return go(ProjCfg3{});
    else return sp.dpw == 1 ? go(ProjCfgE{}) : go(ProjCfgC{});
  });
}

// B[n] = (addend ? addend : 0) + sum over the nsplit slabs; slab sp starts at partial + sp * stride
// (stride < 0: the slabs are dense, stride = n)
// map: where entry idx of the sum goes (default: B[idx]; time slices for a reduce-scatter: kernels.hpp, SliceMap)
// flag: where a non-finite sum is reported (default: the plan's own, which temx_status reads)
static int launch_reduce(temx_plan* pl, const double* partial, int nsplit, int64_t n, double* B,
                         hipStream_t st, int64_t stride = -1, const double* addend = nullptr,
                         const SliceMap& map = SliceMap(), int* flag = nullptr) {
  if (stride < 0) stride = n;
  if (flag == nullptr) flag = static_cast<int*>(pl->flag.p);
  if (nsplit <= 16 && n >= 32768) {   // many entries, few slabs: one thread per entry (same bits)
    const dim3 grid((unsigned)((n + 255) / 256));
    if (nsplit <= 2)
      hipLaunchKernelGGL(reduce_partials_flat_kernel<2>, grid, dim3(256), 0, st, partial, nsplit, stride, n, addend, B, flag, map);
    else if (nsplit <= 4)
      hipLaunchKernelGGL(reduce_partials_flat_kernel<4>, grid, dim3(256), 0, st, partial, nsplit, stride, n, addend, B, flag, map);
    else if (nsplit <= 8)
      hipLaunchKernelGGL(reduce_partials_flat_kernel<8>, grid, dim3(256), 0, st, partial, nsplit, stride, n, addend, B, flag, map);
    else
      hipLaunchKernelGGL(reduce_partials_flat_kernel<16>, grid, dim3(256), 0, st, partial, nsplit, stride, n, addend, B, flag, map);
    HIPCHK(hipGetLastError());
    return TEMX_OK;
  }
  const int64_t blocks = (n + 15) / 16;
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((unsigned)blocks), dim3(256), 0, st, partial, nsplit, stride, n,
                     addend, B, flag, map);
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

// out[f][r][d] = sum over the slabs of the first `rows` of each field's `rows_in` rows (kernels.hpp)
static int launch_reduce_rows(temx_plan* pl, const double* partial, int nsplit, int64_t stride, int nf, int rows_in,
                              int rows, int64_t D, double* out, hipStream_t st) {
  const int64_t n = (int64_t)nf * rows * D;
  if (nsplit > 16)
    hipLaunchKernelGGL(reduce_rows_wide_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, partial, nsplit, stride,
                       nf, rows_in, rows, D, out, static_cast<int*>(pl->flag.p));
  else
    hipLaunchKernelGGL(reduce_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, partial, nsplit, stride,
                       nf, rows_in, rows, D, out, static_cast<int*>(pl->flag.p));
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

static int launch_solve(temx_plan* pl, const double* B, int NF, int64_t D, double* C, double* Xb,
                        hipStream_t st) {
  if (pl->K <= 64) {   // two small MFMA GEMMs per d-tile
    const int nmb = (pl->M + 3) / 4;
    // slices of the output latitudes: every slice recomputes the coefficients (TB^2 MFMAs), so slices
    // are as tall as the LDS image allows (SOLVE_MB) unless the grid would leave most of the chip idle
    const int gx = (int)(((D + 15) / 16 + 3) / 4);
    int mbs = SOLVE_MB;
    while (mbs > 4 && (int64_t)gx * NF * ((nmb + mbs - 1) / mbs) < pl->num_cu / 2) mbs -= 4;
    dim3 grid((unsigned)gx, NF, Xb ? (nmb + mbs - 1) / mbs : 1);
    return dispatch(TBValues{}, pl->TB, [&](auto tb) {
      constexpr int TBv = decltype(tb)::value;
      const size_t slds = ((size_t)TBv * TBv + (size_t)SOLVE_MB * TBv) * 16 * sizeof(double);
      return launch_lds<solve_mfma_kernel<TBv>>(pl->device, grid, dim3(256), slds, st, B, pl->K, pl->M, D, pl->gblk.d(),
                                                pl->ypblk.d(), C, Xb, mbs);
    });
  }
  // 16 waves per block (the solve is latency bound: one round of dot products per phase); slices of
  // 64 output latitudes = one zonal-mean output per thread
  const int ms = Xb ? (pl->M + 63) / 64 : 1;
  dim3 grid((unsigned)((D + 15) / 16), NF, ms);
  const size_t slds = (size_t)2 * pl->K4 * 17 * sizeof(double);
  return launch_lds<solve_kernel, 160 * 1024>(pl->device, grid, dim3(1024), slds, st, B, pl->K, pl->K4, pl->M, D,
      pl->Ginv.d(), pl->Qp.d(), C, Xb);
}

template <typename T, int MODE, int KIND>
static int launch_eddy_t(temx_plan* pl, const FieldPtrs<4>& fp, const double* C, double* partial,
                         const Split& sp, const EddyOut& eo, hipStream_t st) {
  constexpr int NFR = (KIND == 1 || KIND == 3) ? 3 : 4;
  return dispatch(DpwValues{}, sp.dpw, [&](auto dpw) {
    return dispatch(TBValues{}, pl->TB, [&](auto tb) {
      constexpr int DPW = decltype(dpw)::value, TBv = decltype(tb)::value;
      const size_t lds = ((size_t)DPW * NFR * TBv * 64 + 8 * EDDY_GR * TBv * 16) * sizeof(double);
      return launch_lds<eddy_kernel<T, TBv, MODE, DPW, KIND>>(pl->device, dim3(sp.grid), dim3(512), lds, st, fp, pl->N, pl->D,
                                                              pl->K, pl->yblk.d(), pl->nchunk, pl->colscale.d(), C, partial,
                                                              sp.nsplit, sp.ndt, eo);
    });
  });
}

// native-grid reconstruction out[row][d] = sum_l Y0[row0 + row][l] C[l][d] for rows [row0, row0 + nrows),
// row0 a multiple of 16 (whole chunks of the blocked Y0 copy); out is compact [nrows][D]
static int launch_recon(temx_plan* pl, int64_t D, const double* C, double* out, hipStream_t st,
                        int64_t row0 = 0, int64_t nrows = -1) {
  if (nrows < 0) nrows = pl->N - row0;
  const int64_t nch = (nrows + 15) / 16;
  const double* yb0 = pl->yblk.d() + (row0 / 4) * pl->stride * 16;
  Split sp = choose_split(D, nch, 2 * pl->num_cu);
  dim3 grid(sp.grid), block(256);
  if (pl->large) {   // one pass per slice of 64 harmonics, accumulating into out
    for (int sl = 0; sl < pl->nslice; ++sl)
      hipLaunchKernelGGL(recon_kernel<16>, grid, block, (size_t)4 * 16 * 64 * sizeof(double), st, nrows, D, yb0, pl->stride,
          16 * sl, nch, C + (int64_t)64 * sl * D, out, sl > 0 ? 1 : 0, sp.nsplit, sp.ndt);
    HIPCHK(hipGetLastError());
    return TEMX_OK;
  }
  return dispatch(TBValues{}, pl->TB, [&](auto tb) {
    constexpr int TBv = decltype(tb)::value;
    return launch<recon_kernel<TBv>>(grid, block, (size_t)4 * TBv * 64 * sizeof(double), st, nrows, D, yb0, pl->stride, 0,
        nch, C, out, 0, sp.nsplit, sp.ndt);
  });
}

// B[NF][K][D] = Y0^T {fields}: one projection sweep, or one per slice of 64 harmonics (large L)
template <int NF>
static int project_all(temx_plan* pl, const FieldPtrs<NF>& fp, int dtype, int64_t D, const double* colscale,
                       int sfield, const Split& sp, double* B, hipStream_t st) {
  int rc;
  if (!pl->large) {
    if ((rc = launch_project<NF>(pl, fp, dtype, D, colscale, sfield, pl->partial.d(), sp, st))) return rc;
    return launch_reduce(pl, pl->partial.d(), sp.nsplit, (int64_t)NF * pl->K * D, B, st);
  }
  if ((rc = pl->Bs.ensure((size_t)NF * 64 * D * 8))) return rc;
  for (int sl = 0; sl < pl->nslice; ++sl) {
    const int Ks = std::min(64, pl->K - 64 * sl);
    if ((rc = launch_project<NF>(pl, fp, dtype, D, colscale, sfield, pl->partial.d(), sp, st, 16 * sl, Ks))) return rc;
    if ((rc = launch_reduce(pl, pl->partial.d(), sp.nsplit, (int64_t)NF * Ks * D, pl->Bs.d(), st))) return rc;
    for (int f = 0; f < NF; ++f)
      HIPCHK(hipMemcpyAsync(B + ((int64_t)f * pl->K + 64 * sl) * D, pl->Bs.d() + (int64_t)f * Ks * D,
                            (size_t)Ks * D * 8, hipMemcpyDeviceToDevice, st));
  }
  return TEMX_OK;
}

// ------------------------------------------------------------------------------------------------
// latitude classes and mirror pairs: the tolerance, and the work cuts on the device (class_tables.hpp)
// ------------------------------------------------------------------------------------------------
static double sym_tol_deg(double dflt) {
  // Two columns share a latitude class (or pair up) when their |lat| agree to within `tol` degrees; the members are
  // then treated as sitting exactly at the class latitude (the mean of its members), which perturbs a basis row by
  // about L tol (in radians) of its size.  The default, 1e-11 degrees, keeps that below 1e-11 -- a tenth of the fp64
  // parity tolerance -- and covers what asin / round-off leave on grids whose latitudes are equal in exact
  // arithmetic (the natural construction of the cubed sphere is off by ~1e-12 degrees at ne240; round 3 used 1e-12
  // and a grid generator that mirrored the hemispheres bit for bit).  TEMX_LAT_TOL_F32 (fp32 fields: results are
  // compared to 2e-5) widens it to 1e-8 degrees; TEMX_SYM_TOL_DEG in the environment sets it outright, for grids
  // whose files carry noisier latitudes.
  double tol = dflt;
  if (const char* e = getenv("TEMX_SYM_TOL_DEG")) {
    const double t = atof(e);
    if (t > 0.0 && t < 1e-3) tol = t;
  }
  return tol;
}

// work_cuts on the device, one buffer per (pieces, alignment): of the full table ...
static int cached_cuts(std::map<int, DevBuf>& cache, const std::vector<int>& gbatch0, int64_t ngroups, int64_t nbatches,
                       int nsub, bool group_aligned, const int2** out) {
  const int key = group_aligned ? -nsub : nsub;
  auto it = cache.find(key);
  if (it == cache.end()) {
    DevBuf b;
    if (int rc = upload(b, work_cuts(gbatch0, ngroups, nbatches, nsub, group_aligned))) return rc;
    it = cache.emplace(key, b).first;
  }
  *out = static_cast<const int2*>(it->second.p);
  return TEMX_OK;
}
static int class_cuts_dev(temx_plan* pl, int nsub, const int2** out, bool group_aligned = false) {
  return cached_cuts(pl->csplits, pl->gbatch0, pl->cgroups, pl->cbatches, nsub, group_aligned, out);
}
// ... and of the subsample of the single sweep's pre-pass (sub), always group-aligned
static int os_cuts_dev(temx_plan* pl, bool sub, int nsub, const int2** out) {
  if (!sub) return class_cuts_dev(pl, nsub, out, true);
  return cached_cuts(pl->csplits_s, pl->sgbatch0, pl->sgroups, pl->sbatches, nsub, true, out);
}

// (TEMX_CLS_E_WPS, TEMX_CLS_OP_WPS and TEMX_CLS_MINCHUNK enter the cuts: tem_layout.hpp)
#ifndef TEMX_CLS_E_PD
#define TEMX_CLS_E_PD 2
#endif
#ifndef TEMX_CLS_OP_PD
#define TEMX_CLS_OP_PD 3
#endif
#ifndef TEMX_CLS_OP_PD_F32
#define TEMX_CLS_OP_PD_F32 6
#endif
#ifndef TEMX_CLS_E_PD_F32
#define TEMX_CLS_E_PD_F32 4
#endif
#ifndef TEMX_CLS_Q_PD_F32
#define TEMX_CLS_Q_PD_F32 2
#endif
constexpr int CLS_PROJ_E_PD = TEMX_CLS_E_PD;   // one field per wave (CLS_PROJ_E_WPS: tem_layout.hpp)
// X batches a wave of the class project sweep holds (PD - 1 in flight).  A batch of fp32 carries half
// the bytes of an fp64 one in half the registers, so fp32 inputs get rings twice as deep: the same
// bytes in flight per wave.
template <typename T>
constexpr int cls_proj_pd(bool op, int nfw) {
  constexpr bool f32 = sizeof(T) == 4;
  return op ? (f32 ? TEMX_CLS_OP_PD_F32 : TEMX_CLS_OP_PD)
            : (nfw == 1 ? (f32 ? TEMX_CLS_E_PD_F32 : CLS_PROJ_E_PD) : (f32 ? TEMX_CLS_Q_PD_F32 : 2));
}

template <int NF>
static int launch_project_cls(temx_plan* pl, const FieldPtrs<NF>& fp, int dtype, int64_t D,
                              const double* colscale, int sfield, double* partial, const Split& sp,
                              hipStream_t st) {
  return by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    const int2* cuts = nullptr;
    if (int rc = class_cuts_dev(pl, sp.nsplit, &cuts)) return rc;
    auto go = [&](auto nfw, auto wps) {
      return dispatch(TBSValues{}, pl->TBS, [&](auto tbs) {
        constexpr int NFW = decltype(nfw)::value, WPS = decltype(wps)::value;
        return launch<project_cls_kernel<T, NF, NFW, decltype(tbs)::value, WPS, cls_proj_pd<T>(false, NFW), false>>(
            dim3(sp.grid), dim3(256), 0, st, fp, D, pl->K, pl->ycls.d(), static_cast<const int4*>(pl->crow.p), cuts, colscale,
            sfield, partial, sp.nsplit, sp.ndt, (double*)nullptr);
      });
    };
    // one field per wave (NF = 4: small ragged D, one d-tile per workgroup), or all of them
    return NF == 1 || sp.dpw == 1 ? go(Int<1>{}, Int<CLS_PROJ_E_WPS>{}) : go(Int<NF>{}, Int<2>{});
  });
}

// KIND 0: (u, v, T, omega) -> csum; KIND 1: (q, v, omega) -> csq
template <int KIND>
static int launch_sweep_op(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, double* partial, const Split& sp,
                           hipStream_t st) {
  double* sums = KIND == 0 ? pl->csum.d() : pl->csq.d();
  return by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    const int2* cuts = nullptr;
    if (int rc = class_cuts_dev(pl, sp.nsplit, &cuts, true)) return rc;
    dim3 grid(sp.grid), block(256);
    // the tracer sweep (42 accumulators) runs two waves per SIMD: a ring of 2 batches keeps it inside 256 registers
    constexpr int PDv = KIND == 1 ? (sizeof(T) == 4 ? 4 : 2) : (sizeof(T) == 4 ? TEMX_CLS_OP_PD_F32 : TEMX_CLS_OP_PD);
    // loads of 1 row x 64 columns (sweep_opr_kernel, kernels_op2.hpp) unless the last workgroup column would be
    // mostly padding (D = 72: 64 + 8) or TEMX_OP_MAP=tile asks for the tile form (A/B)
    const int64_t wcols = (pl->D + 63) / 64 * 64;
    // fp64 only: with fp32 inputs the tile form measured faster (ne240 x 128 x 1: 1.77 vs 2.08 ms, ne120 x 72 x 30: 7.2 vs 7.5)
    const bool row_map = sizeof(T) == 8 && !pl->op_tile && wcols * 100 <= pl->D * 115;
    constexpr int PDr = 2;
    return dispatch(TBSValues{}, pl->TBS, [&](auto tbs) {
      constexpr int TBSv = decltype(tbs)::value;
      if (row_map)
        return launch<sweep_opr_kernel<double, TBSv, PDr, KIND>>(grid, block, 0, st, fp, pl->D, pl->K, pl->ycls.d(),
                                                                 static_cast<const int4*>(pl->crow.p), cuts, pl->colscale.d(),
                                                                 partial, sp.nsplit, sp.ndt, sums);
      return launch<sweep_op_kernel<T, TBSv, PDv, KIND>>(grid, block, 0, st, fp, pl->D, pl->K, pl->ycls.d(),
          static_cast<const int4*>(pl->crow.p), cuts, pl->colscale.d(), partial, sp.nsplit, sp.ndt, sums);
    });
  });
}

// TEM + one tracer in one sweep (kernels_op2.hpp): (u, v, T, omega, q) -> csum, csq, 10 slabs per split
template <typename T>
static int launch_sweep_opw2_t(temx_plan* pl, const FieldPtrs<5>& fp, double* partial, const Split& sp, hipStream_t st) {
  const int2* cuts = nullptr;
  if (int rc = class_cuts_dev(pl, sp.nsplit * 4, &cuts, true)) return rc;
  dim3 grid(sp.grid), block(256);
  constexpr int PDv = sizeof(T) == 4 ? TEMX_CLS_OP_PD_F32 : TEMX_CLS_OP_PD;
  return dispatch(TBSValues{}, pl->TBS, [&](auto tbs) {
    return launch<sweep_opw_kernel<T, decltype(tbs)::value, PDv, 2>>(grid, block, 0, st, fp, pl->D, pl->K, pl->ycls.d(),
        static_cast<const int4*>(pl->crow.p), cuts, pl->colscale.d(), partial, sp.nsplit, sp.ndt, pl->csum.d(),
        pl->csq.d());
  });
}

template <typename T, int MODE, int KIND>
static int launch_eddy_cls_t(temx_plan* pl, const FieldPtrs<4>& fp, const double* C, double* partial,
                             const Split& sp, const EddyOut& eo, hipStream_t st) {
  constexpr int NFR = KIND == 0 ? 4 : 3;
  return dispatch(DpwValues{}, sp.dpw, [&](auto dpw) {
    constexpr int DPW = decltype(dpw)::value;
    const int2* cuts = nullptr;
    if (int rc = class_cuts_dev(pl, sp.nsplit * (8 / DPW), &cuts)) return rc;
    return dispatch(TBSValues{}, pl->TBS, [&](auto tbs) {
      constexpr int TBSv = decltype(tbs)::value;
      const size_t lds = ((size_t)DPW * NFR * 2 * TBSv * 64 + 8 * 2 * TBSv * 16) * sizeof(double);
      return launch_lds<eddy_cls_kernel<T, TBSv, MODE, DPW, KIND>>(pl->device, dim3(sp.grid), dim3(512), lds, st, fp, pl->D,
          pl->K, pl->K4, pl->ycls.d(), static_cast<const int4*>(pl->crow.p), cuts, pl->colscale.d(), C, partial, sp.nsplit,
          sp.ndt, eo);
    });
  });
}

template <int KIND>
static int launch_flux_cls(temx_plan* pl, const double* C, double* partial, const Split& sp, hipStream_t st) {
  return dispatch(DpwValues{}, sp.dpw, [&](auto dpw) {
    return dispatch(TBSValues{}, pl->TBS, [&](auto tbs) {
      constexpr int DPW = decltype(dpw)::value, TBSv = decltype(tbs)::value;
      const size_t lds = ((size_t)DPW * 4 * 2 * TBSv * 64 + 8 * 2 * TBSv * 16) * sizeof(double);
      return launch_lds<flux_cls_kernel<TBSv, DPW, KIND>>(pl->device, dim3(sp.grid), dim3(512), lds, st, pl->D, pl->K,
          pl->K4, pl->ycls.d(), pl->csum.d(), pl->csq.d(), pl->ccnt.d(), pl->cgroups, C, partial, sp.nsplit, sp.ndt);
    });
  });
}

// ---- large-L class path ----------------------------------------------------------------------------
// sweep 1: the class sums of the four fields and of u v, u omega, v T (no projection)
static int launch_class_sums(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, hipStream_t st) {
  const Split& sp = pl->sp_cproj4;
  const int2* cuts = nullptr;
  if (int rc = class_cuts_dev(pl, sp.nsplit, &cuts, true)) return rc;
  dim3 grid(sp.grid), block(256);
  return by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch<project_cls_kernel<T, 4, 4, 2, TEMX_CLS_OP_WPS, cls_proj_pd<T>(true, 4), true, false>>(grid, block, 0,
        st, fp, pl->D, pl->K, (const double*)nullptr, static_cast<const int4*>(pl->crow.p), cuts, pl->colscale.d(), 2,
        (double*)nullptr, sp.nsplit, sp.ndt, pl->csum.d());
  });
}

// B[NQ][K][D] = sum over classes of Y_l (S_N +- S_S) for NQ sums of the records in rec, slice by slice
template <int NQ>
static int project_sums(temx_plan* pl, const double* rec, int RS, int row0, double* B, hipStream_t st) {
  const Split& sp = pl->sp_cflux;
  const int64_t D = pl->D;
  dim3 grid(sp.grid), block(512);
  int rc;
  for (int sl = 0; sl < pl->nslice; ++sl) {
    const int Ks = std::min(64, pl->K - 64 * sl);
    rc = dispatch(DpwValues{}, sp.dpw, [&](auto dpw) {
      constexpr int DPW = decltype(dpw)::value;
      const size_t lds = ((size_t)DPW * NQ * 16 * 64 + 8 * 256) * sizeof(double);
      return launch_lds<sums_project_kernel<NQ, DPW>>(pl->device, grid, block, lds, st, D, pl->K, 64 * sl,
                                                      pl->ycls_l.d() + sl * pl->ycls_lstride, rec, RS, row0, pl->cgroups,
                                                      pl->partial.d(), sp.nsplit, sp.ndt);
    });
    if (rc) return rc;
    if ((rc = launch_reduce(pl, pl->partial.d(), sp.nsplit, (int64_t)NQ * Ks * D, pl->Bs.d(), st))) return rc;
    for (int q = 0; q < NQ; ++q)
      HIPCHK(hipMemcpyAsync(B + ((int64_t)q * pl->K + 64 * sl) * D, pl->Bs.d() + (int64_t)q * Ks * D,
                            (size_t)Ks * D * 8, hipMemcpyDeviceToDevice, st));
  }
  return TEMX_OK;
}

static int launch_flux_large(temx_plan* pl, const double* C, hipStream_t st) {
  const Split& sp = pl->sp_lflux;
  dim3 grid(sp.grid), block(512);
  return dispatch(SliceValues{}, pl->nslice, [&](auto ns) {
    constexpr int NS = decltype(ns)::value;
    const size_t lds = ((size_t)NS * 4 * 16 * 64 + 8 * 256) * sizeof(double);
    return launch_lds<flux_large_kernel<NS>>(pl->device, grid, block, lds, st, pl->D, pl->K, pl->K4, pl->ycls_l.d(),
        pl->ycls_lstride, pl->csum.d(), pl->ccnt.d(), pl->cgroups, C, pl->pbuf.d(), sp.nsplit, sp.ndt);
  });
}

template <int NF>
static int launch_project_sym(temx_plan* pl, const FieldPtrs<NF>& fp, int dtype, int64_t D,
                              const double* colscale, int sfield, double* partial, const Split& sp,
                              hipStream_t st) {
  return by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto go = [&](auto nfw, auto wps) {
      return dispatch(TBSValues{}, pl->TBS, [&](auto tbs) {
        return launch<project_sym_kernel<T, NF, decltype(nfw)::value, decltype(tbs)::value, decltype(wps)::value>>(
            dim3(sp.grid), dim3(256), 0, st, fp, D, pl->K, pl->ysym.d(), static_cast<const int*>(pl->rows.p), pl->npg,
            pl->npg_alloc * 4, colscale, sfield, partial, sp.nsplit, sp.ndt);
      });
    };
    // small ragged D: one d-tile per workgroup, one field per wave
    return NF == 4 && sp.dpw == 1 ? go(Int<1>{}, Int<SYM_PROJ_E_WPS>{}) : go(Int<NF>{}, Int<2>{});
  });
}

template <typename T, int MODE, int KIND>
static int launch_eddy_sym_t(temx_plan* pl, const FieldPtrs<4>& fp, const double* C, double* partial,
                             const Split& sp, const EddyOut& eo, hipStream_t st) {
  constexpr int NFR = KIND == 0 ? 4 : 3;
  return dispatch(DpwValues{}, sp.dpw, [&](auto dpw) {
    return dispatch(TBSValues{}, pl->TBS, [&](auto tbs) {
      constexpr int DPW = decltype(dpw)::value, TBSv = decltype(tbs)::value;
      const size_t lds = ((size_t)DPW * NFR * 2 * TBSv * 64 + 8 * 2 * TBSv * 16) * sizeof(double);
      return launch_lds<eddy_sym_kernel<T, TBSv, MODE, DPW, KIND>>(pl->device, dim3(sp.grid), dim3(512), lds, st, fp, pl->D,
          pl->K, pl->K4, pl->ysym.d(), static_cast<const int*>(pl->rows.p), pl->npg, pl->npg_alloc * 4, pl->npair,
          pl->colscale.d(), C, partial, sp.nsplit, sp.ndt, eo);
    });
  });
}

// The fused second sweep reads ONE set of Y0 blocks for the reconstruction and for the projection, so it
// serves neither K > 64 nor weights mode (projection rows scaled by 4 pi w, reconstruction rows not).
static inline bool unfused_stage2(const temx_plan* pl) { return pl->large || pl->weighted; }
// what tem_layout.hpp reads of a plan
static TemDims tem_dims(const temx_plan* pl) {
  TemDims d;
  d.N = pl->N; d.nchunk = pl->nchunk; d.K = pl->K; d.K4 = pl->K4; d.M = pl->M; d.num_cu = pl->num_cu;
  d.nlev = pl->nlev; d.nt = pl->nt;
  d.unfused_stage2 = unfused_stage2(pl); d.lcls = pl->lcls; d.cls = pl->cls; d.sym = pl->sym;
  d.cgroups = pl->cgroups; d.cbatches = pl->cbatches; d.npg = pl->npg;
  return d;
}

static inline hipStream_t S_(void* s) { return static_cast<hipStream_t>(s); }
static inline const Split& eddy_split(const temx_plan* pl) {
  return pl->cls ? pl->sp_ceddy : (pl->sym ? pl->sp_seddy : pl->sp_eddy);
}
static inline int eddy_slabs(const temx_plan* pl) {   // partial slabs the eddy sweep writes per product
  if (pl->cls) return pl->sp_ceddy.nsplit;           // the class sweep adds its waves up in LDS first
  return eddy_split(pl).nsplit * (8 / eddy_split(pl).dpw);
}
static inline bool sym_project(const temx_plan* pl, int nf) {   // paired project sweep needs d-quads
  return pl->sym && (nf == 4 ? pl->sp_sproj4.nsplit : pl->sp_sproj1.nsplit) > 0;
}

template <int KIND>
static int run_eddy(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, const double* C, double* partial,
                    const EddyOut* eo, hipStream_t st) {
  const EddyOut none{};
  return by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    auto go = [&](auto mode) {       // MODE 1: the sweep also writes the native eddy fields *eo
      constexpr int MODE = decltype(mode)::value;
      const EddyOut& o = MODE ? *eo : none;
      if (pl->cls) return launch_eddy_cls_t<T, MODE, KIND>(pl, fp, C, partial, pl->sp_ceddy, o, st);
      if (pl->sym) return launch_eddy_sym_t<T, MODE, KIND>(pl, fp, C, partial, pl->sp_seddy, o, st);
      return launch_eddy_t<T, MODE, KIND>(pl, fp, C, partial, pl->sp_eddy, o, st);
    };
    return eo ? go(Int<1>{}) : go(Int<0>{});
  });
}

static FieldPtrs<4> four(const void* a, const void* b, const void* c, const void* d) {
  FieldPtrs<4> fp;
  fp.p[0] = a; fp.p[1] = b; fp.p[2] = c; fp.p[3] = d;
  return fp;
}

// ---- single-sweep form ---------------------------------------------------------------------------------
// The class-sum stream costs sweep 1 2.2 of its 11.1 ms and feeds a 1.8 ms flux kernel.  This
// form needs neither: ONE sweep projects the four fields up to degree 2L and the three products up to degree
// L (sweep_os_kernel), and the eddy-product sums follow from the Legendre product linearisation
// (os_contract_kernel).  A band-limited reference of low degree, fitted to a subsample of class-groups in a
// short pre-pass with the same kernel, is subtracted first so that no term is a difference of large numbers
// (tools/proto/single_sweep_numerics.py).  Used by temx_tem_run only (the staged, all-reducible stages keep the
// class-sum path).

// tables that depend on the grid and L only (built once per plan, at the first eligible temx_plan_set_tem)
static int build_os_tables(temx_plan* pl) {
  if (pl->os_built) return TEMX_OK;
  const int K = pl->K, L = pl->L;
  const int KX = 2 * L + 1;
  const int TBX = pl->TBS == 7 ? 13 : (pl->TBS == 4 ? 8 : 4);      // blocks per parity of the degree-2L basis (zero padded)
  const int KR = std::min(16, K);
  pl->KX = KX;
  pl->TBX = TBX;
  pl->KR = KR;
  int rc;
  // subsample of class-groups for the reference fit (TEMX_OPT_OS_SUBSAMPLE / env TEMX_OS_SUBSAMPLE: groups kept)
  const char* ess = getenv("TEMX_OS_SUBSAMPLE");
  const ClassSubsample ss = class_subsample(pl->h_crow, pl->h_xc, pl->gbatch0, pl->cgroups, ess ? std::max(4, atoi(ess)) : pl->os_keep);
  pl->sgbatch0 = ss.gbatch0;
  pl->sgroups = ss.ngroups;
  pl->sbatches = ss.nbatch;
  if ((rc = upload(pl->crow_s, ss.crow))) return rc;
  // one row table per side, for the full table and for the subsample (sweep_os2_kernel: a wave per class side)
  for (int sub = 0; sub < 2; ++sub) {
    SideTables stb;
    if (sub) build_side_tables(ss.crow, ss.gbatch0, ss.ngroups, stb);
    else build_side_tables(pl->h_crow, pl->gbatch0, pl->cgroups, stb);
    for (int sd = 0; sd < 2; ++sd) {
      if ((rc = upload(pl->side_crow[sub][sd], stb.crow[sd]))) return rc;
      if ((rc = upload(pl->side_gfirst[sub][sd], stb.gfirst[sd]))) return rc;
    }
  }
  // basis up to degree 2L at the class latitudes of the full table and of the subsample, Y basis (no
  // re-orthogonalisation: these are raw projections)
  {
    std::vector<double> nx((size_t)8 * TBX + 8, 0.0);
    for (int l = 0; l < KX; ++l) nx[(size_t)l] = std::sqrt((2.0 * l + 1.0) / (4.0 * M_PI));
    DevBuf nd, xs;
    if (!(rc = upload(nd, nx)) && !(rc = upload(xs, ss.xc)) && !(rc = pl->ycx.ensure((size_t)(pl->cgroups + 1) * 2 * TBX * 16 * 8)) &&
        !(rc = pl->ycx_s.ensure((size_t)(pl->sgroups + 1) * 2 * TBX * 16 * 8))) {
      hipLaunchKernelGGL(cls_basis_kernel<512>, dim3((unsigned)((pl->cls_npad + 255) / 256)), dim3(256), 0, 0, pl->xc.d(),
                         pl->ncls, pl->cls_npad, KX, TBX, nd.d(), (const double*)nullptr, pl->ycx.d());
      const int64_t np = (pl->sgroups + 1) * 4;
      hipLaunchKernelGGL(cls_basis_kernel<512>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, 0, xs.d(), pl->sgroups * 4,
                         np, KX, TBX, nd.d(), (const double*)nullptr, pl->ycx_s.d());
      const hipError_t e = hipDeviceSynchronize();
      if (e != hipSuccess) rc = fail(TEMX_EHIP, "extended class basis failed: %s", hipGetErrorString(e));
    }
    nd.release();
    xs.release();
    if (rc) return rc;
  }
  // Gram matrix of the subsample, degree < KR, and its inverse
  {
    pl->h_Gs = subsample_gram(pl->h_xc, pl->h_cnt, pl->cgroups, ss.S, KR);
    std::vector<long double> Li;
    std::vector<double> Gi((size_t)KR * KR, 0.0);
    if (spd_factor(pl->h_Gs.data(), KR, Li) == 0) {
      inverse_from_factor(Li, KR, Gi.data());
    } else if (pl->ext_G) {
      // A rank of an ncol-sharded job owns a band of latitudes, which need not determine the fit on its own:
      // the job's subsample is the union over the ranks, its Gram matrix comes through
      // temx_plan_set_os_matrices (the sweeps refuse to run before that).
      pl->os_need_global = true;
    } else {
      return fail(TEMX_ERANK, "the subsample of latitude classes does not determine a degree-%d reference", KR - 1);
    }
    if ((rc = upload(pl->Gsinv, Gi))) return rc;
  }
  // Gauss-Legendre nodes for the transform form of the product linearisation (exact for degree 4L)
  {
    const int nq = 2 * L + 2;
    pl->NQ = nq;
    const QuadBasis qb = quadrature_basis(nq, KX);
    pl->h_Yq.assign(qb.Y.begin(), qb.Y.end());                              // (Yq[q][k])
    if ((rc = upload(pl->gaunt, pl->h_Yq))) return rc;
    if ((rc = upload(pl->wq2, std::vector<double>(qb.w2.begin(), qb.w2.end())))) return rc;
  }
  // Gx[l][k] = sum over the native columns of Y_l Y_k, l < K, k < KX (per latitude class; host threads)
  pl->h_Gx = extended_gram(pl->h_xc, pl->h_cnt, pl->ncls, K, KX, (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())));
  pl->h_Gx_own = pl->h_Gx;
  if ((rc = upload(pl->Gx, pl->h_Gx))) return rc;
  pl->os_built = true;
  return os_upload_blocks(pl);
}

// the matrices of the single sweep's contraction as MFMA operand blocks: after build_os_tables, and again whenever
// one of them changes (temx_plan_finalize / refine: T, G2inv, G; temx_plan_set_os_matrices: Gx)
static int os_upload_blocks(temx_plan* pl) {
  if (pl->h_T.empty() || pl->h_Ginv.empty() || pl->h_G.empty() || pl->h_Yq.empty() || pl->h_Gx.empty()) return TEMX_OK;
  const int K = pl->K, KX = pl->KX, KR = pl->KR, NQ = pl->NQ;
  const int NBK = pl->TB, NBX = 2 * pl->TBX;
  if (4 * NBK < K || 4 * NBX < KX || 4 * NBX < NQ) return fail(TEMX_EUNSUPPORTED, "single-sweep contraction: no instantiation for L = %d", pl->L);
  std::vector<double> blk;
  size_t off[9];
  const double* T = pl->h_T.data();
  const double* Yq = pl->h_Yq.data();
  off[0] = blk.size(); append_blocks16(blk, T, K, K, K, true, NBK, NBK);                    // T^T
  off[1] = blk.size(); append_blocks16(blk, pl->h_Ginv.data(), K, K, K, false, NBK, NBK);   // G2inv
  off[2] = blk.size(); append_blocks16(blk, T, K, K, K, false, NBK, NBK);                   // T
  off[3] = blk.size(); append_blocks16(blk, pl->h_G.data(), K, KR, K, false, NBK, 4);       // G[:, :KR]
  off[4] = blk.size(); append_blocks16(blk, Yq, NQ, K, KX, false, NBX, NBK);                // Yq[:, :K]
  off[5] = blk.size(); append_blocks16(blk, Yq, NQ, KX, KX, false, NBX, NBX);               // Yq
  off[6] = blk.size(); append_blocks16(blk, Yq, K, NQ, KX, true, NBK, NBX);                 // Yq[:, :K]^T
  off[7] = blk.size(); append_blocks16(blk, Yq, KX, NQ, KX, true, NBX, NBX);                // Yq^T
  off[8] = blk.size(); append_blocks16(blk, pl->h_Gx.data(), K, KX, KX, false, NBK, NBX);   // Gx
  HIPCHK(hipDeviceSynchronize());              // (a launch in flight may still read the old blocks)
  if (int rc = upload(pl->oscblk, blk.data(), blk.size() * 8)) return rc;
  const double* b = pl->oscblk.d();
  pl->osc = OscMats{b + off[0], b + off[1], b + off[2], b + off[3], b + off[4], b + off[5], b + off[6], b + off[7], b + off[8]};
  return TEMX_OK;
}

#ifndef TEMX_OS_DEFER
#define TEMX_OS_DEFER 1
#endif
template <typename T, int KIND>
static int launch_sweep_os_t(temx_plan* pl, const FieldPtrs<4>& fp, bool sub, const double* rho, double* partial,
                             const Split& sp, hipStream_t st) {
  using KD = OsKind<KIND>;
  const int2* cuts = nullptr;
  if (int rc = os_cuts_dev(pl, sub, sp.nsplit, &cuts)) return rc;
  dim3 grid(sp.grid), block(256);
  constexpr int NBR = OS_NBR;
  constexpr int PDv = sizeof(T) == 4 ? 4 : 2;       // (a 3-deep ring measured slower for the tracer kind: 8.7 vs 8.4 ms)
  constexpr int DF = TEMX_OS_DEFER;                 // projection of a finished class-group spread over the next 4 batches
  // loads of 1 row x 64 columns (sweep_osr_kernel, the default) or of 4 rows x 16 columns (TEMX_OS_MAP=tile, A/B)
  const bool tile_map = pl->os_tile;
  double* px = partial;
  // (the reference pre-pass needs the first KR rows of px only: pp == NULL tells the kernels to store nothing else --
  //  146 x 8 B per lane and workgroup otherwise, 150 MB at ne120 x 72 x 30 for a sweep that reads 240 MB)
  double* pp = sub ? nullptr : partial + (int64_t)sp.nsplit * KD::NFX * pl->KX * pl->D;
  int rc = TEMX_OK;
  const bool listed = dispatch_strict(OsPairs{}, pl->TBS, pl->TBX, rc, [&](auto pair) {
    constexpr int TBSv = decltype(pair)::first, TBXv = decltype(pair)::second;
    if constexpr (KIND == 3) {
      if (tile_map) return fail(TEMX_EUNSUPPORTED, "two tracers per sweep: row-map sweeps only");
    }
    if constexpr (KIND != 3) if (tile_map) {
      constexpr size_t lds = sweep_os_lds(TBSv, TBXv, KD::NF, KD::NP, KD::NPR, DF);
      return launch_lds<sweep_os_kernel<T, TBSv, TBXv, NBR, PDv, KIND, DF>>(pl->device, grid, block, lds, st, fp, pl->D,
          pl->K, pl->KX, sub ? pl->ycx_s.d() : pl->ycx.d(), static_cast<const int4*>(sub ? pl->crow_s.p : pl->crow.p), cuts,
          pl->colscale.d(), rho, pl->KR, px, pp, sp.nsplit, sp.ndt);
    }
    if (sizeof(T) == 4) {   // fp32 inputs: two waves per SIMD (kernels_op2.hpp, sweep_os2_kernel)
      if (pl->cls_max_side > 8 * TEMX_F32_SIDE_CAP)
        return fail(TEMX_EUNSUPPORTED, "single sweep of fp32 fields: a latitude class of this plan has %lld members on one "
                    "side, and the sweep sums a side in fp32; create the plan with TEMX_LAT_TOL_F32",
                    (long long)pl->cls_max_side);
      constexpr size_t lds = sweep_os2_lds(TBSv, TBXv, KD::NF, KD::NP, KD::NPR, DF);
      const int si = sub ? 1 : 0;
      return launch_lds<sweep_os2_kernel<float, TBSv, TBXv, NBR, 2, KIND>>(
          pl->device, grid, dim3(512), lds, st, fp, pl->D, pl->K, pl->KX, sub ? pl->ycx_s.d() : pl->ycx.d(),
          static_cast<const int4*>(pl->side_crow[si][0].p), static_cast<const int4*>(pl->side_crow[si][1].p),
          static_cast<const int*>(pl->side_gfirst[si][0].p), static_cast<const int*>(pl->side_gfirst[si][1].p),
          cuts, pl->colscale.d(), rho, pl->KR, px, pp, sp.nsplit, sp.ndt);
    }
    constexpr size_t lds = sweep_osr_lds(TBSv, TBXv, KD::NF, KD::NP, KD::NPR, DF);
    static_assert(lds <= 163840, "the single sweep's workgroup fits the LDS of a compute unit");
    auto go = [&](auto handoff) {     // 0: two workgroup barriers per group, 1: LDS flags
      return launch_lds<sweep_osr_kernel<double, TBSv, TBXv, NBR, 2, KIND, decltype(handoff)::value>>(pl->device, grid,
          block, lds, st, fp, pl->D, pl->K, pl->KX, sub ? pl->ycx_s.d() : pl->ycx.d(),
          static_cast<const int4*>(sub ? pl->crow_s.p : pl->crow.p), cuts, pl->colscale.d(), rho, pl->KR, px, pp, sp.nsplit,
          sp.ndt, static_cast<int*>(pl->flag.p) + 1);
    };
    return pl->os_barrier ? go(Int<0>{}) : go(Int<1>{});
  });
  return listed ? rc : fail(TEMX_EUNSUPPORTED, "single-sweep form: no instantiation for L = %d", pl->L);
}

template <int KIND>
static int launch_sweep_os(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, bool sub, const double* rho, double* partial,
                           const Split& sp, hipStream_t st) {
  return dtype == TEMX_F64 ? launch_sweep_os_t<double, KIND>(pl, fp, sub, rho, partial, sp, st)
                           : launch_sweep_os_t<float, KIND>(pl, fp, sub, rho, partial, sp, st);
}

static bool os_supported(const temx_plan* pl) {
  return os_supported(pl->cls, pl->large, pl->weighted, pl->qbasis, !pl->h_crow.empty(), pl->TBS, pl->L);
}

// the single-sweep forms run for both input types (fp32 inputs take the two-waves-per-SIMD sweep);
// TEMX_SINGLE_SWEEP=0 at plan build selects the class-sum forms
static bool os_active(const temx_plan* pl, int dtype) {
  (void)dtype;
  return pl->os_on;
}

// The snapshots [t0, t0 + nts) the tail (solve, contraction, scan, epilogue) is about to describe.  Everything the
// tail leaves in the plan (C4, zb, Ax, tz ...) then has nlev * nts columns.
static void set_tail(temx_plan* pl, int64_t t0, int64_t nts) {
  if (pl->tt0 != t0 || pl->tnt != nts) pl->c4_valid = pl->os_valid = pl->op_valid = pl->tq_valid = pl->xb_valid = false;
  pl->tt0 = t0;
  pl->tnt = nts;
  pl->tD = (int64_t)pl->nlev * nts;
}
static inline bool tail_is_whole(const temx_plan* pl) { return pl->tt0 == 0 && pl->tnt == pl->nt; }

static int tem_stage3_impl(temx_plan* pl, const double* B3, double* results, double* zonal, hipStream_t st);
static int tem_epilogue(temx_plan* pl, double* results, double* zonal, hipStream_t st);
static int bin_project_op(temx_plan* pl, const void* A, int dtype, int64_t D, double* B, hipStream_t st);
static int bin_zonal_mean(temx_plan* pl, const void* A, int dtype, int64_t D, double* out, int native, hipStream_t st);
static int miss_check(const temx_plan* pl);
static int miss_zonal_mean(temx_plan* pl, const void* A, int dtype, int64_t D, double* out, int native, hipStream_t st);
static int tracer_stage3_impl(temx_plan* pl, const double* Bq2, double* tres, double* tzon, hipStream_t st);

// Time slices of a reduction (kernels.hpp, SliceMap): nsl slices, rows_total rows per slice
static SliceMap slice_map(const temx_plan* pl, int nsl, int64_t rows_total, int64_t row0) {
  SliceMap m;
  if (nsl <= 1) return m;
  m.D = pl->D;
  m.nt = (int)pl->nt;
  m.W = nsl;
  m.chunk = rows_total * pl->nlev * ((pl->nt + nsl - 1) / nsl);
  m.row0 = row0;
  return m;
}

// the contraction on the matrix cores (kernels_osc.hpp): fields, then pairs
template <int NBK>
static int launch_osc_t(temx_plan* pl, const OscFieldsIn& fin, int nf, int nout, double* Bf, double* At, double* ab,
                        const OscPairsIn& pin, int np, double* Bp, int64_t Dt, hipStream_t st) {
  const unsigned gx = (unsigned)((Dt + 15) / 16);       // one workgroup (OSC_W waves) = one d-tile of one field / pair
  hipLaunchKernelGGL((osc_fields_kernel<NBK>), dim3(gx, nf, 2), dim3(OSC_W * 64), (size_t)osc_fields_lds(NBK) * 8, st, fin, pl->osc, pl->K,
                     pl->KX, pl->KR, pl->NQ, Dt, nout, Bf, At, ab, pl->D, (int)pl->tnt, (int)pl->nt, (int)pl->tt0);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL((osc_pairs_kernel<NBK>), dim3(gx, np), dim3(OSC_W * 64), (size_t)osc_pairs_lds(NBK) * 8, st, pin, pl->osc, pl->wq2.d(),
                     pl->K, pl->KX, pl->NQ, Dt, Bp);
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}
static int launch_osc(temx_plan* pl, const OscFieldsIn& fin, int nf, int nout, double* Bf, double* At, double* ab,
                      const OscPairsIn& pin, int np, double* Bp, int64_t Dt, hipStream_t st) {
  if (pl->TB == 13 && pl->TBX == 13) return launch_osc_t<13>(pl, fin, nf, nout, Bf, At, ab, pin, np, Bp, Dt, st);
  if (pl->TB == 8 && pl->TBX == 8) return launch_osc_t<8>(pl, fin, nf, nout, Bf, At, ab, pin, np, Bp, Dt, st);
  if (pl->TB == 4 && pl->TBX == 4) return launch_osc_t<4>(pl, fin, nf, nout, Bf, At, ab, pin, np, Bp, Dt, st);
  return fail(TEMX_EUNSUPPORTED, "single-sweep contraction: no instantiation for L = %d", pl->L);
}

// ---- the single sweep in three steps.  A single process runs them back to back (tem_run_os); an ncol-sharded job
// exchanges between them: (1) -> all-reduce of As (4 x KR x D doubles) -> (2) -> reduce-scatter of proj over time
// -> (3) on the snapshots the rank received.
// 1. reference pre-pass: the same sweep over the subsample of class-groups with a zero reference; As[4][KR][D] =
//    raw sums of the four fields on the first KR harmonics (this rank's rows)
static int os_prepass(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, double* As, hipStream_t st) {
  int rc;
  const int64_t D = pl->D, KD4 = (int64_t)4 * pl->KX * D;
  pl->op_valid = pl->c4_valid = pl->tq_valid = pl->os_valid = false;       // no class sums on this path
  if ((rc = launch_sweep_os<0>(pl, fp, dtype, true, pl->rho0.d(), pl->partial.d(), pl->sp_os_s, st))) return rc;
  return launch_reduce_rows(pl, pl->partial.d(), pl->sp_os_s.nsplit, KD4, 4, pl->KX, pl->KR, D, As, st);
}

// 2. reference coefficients from the (global) subsample sums, the sweep, and its reduction: proj = [4 KX + 3 K] rows
//    (projections of the shifted fields to degree 2L, of their products to degree L), whole ([rows][D]) or cut into
//    nsl time slices ([nsl][rows][nlev][ceil(nt / nsl)], the input of a reduce-scatter)
static int os_sweep(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, const double* As, int nsl, double* proj, hipStream_t st) {
  int rc;
  const int64_t D = pl->D;
  const int64_t KD4 = (int64_t)4 * pl->KX * D, KD3 = (int64_t)3 * pl->K * D;
  pl->op_valid = pl->c4_valid = pl->tq_valid = pl->os_valid = false;
  hipLaunchKernelGGL(os_ref_solve_kernel, dim3((unsigned)((D + 15) / 16), 4), dim3(256), 0, st, As, pl->KR, pl->KR, D,
                     pl->Gsinv.d(), pl->rho.d());
  HIPCHK(hipGetLastError());
  TimedLaunch tl{};
  time_begin(pl, 0, st, tl);
  rc = launch_sweep_os<0>(pl, fp, dtype, false, pl->rho.d(), pl->partial.d(), pl->sp_os, st);
  time_end(pl, 0, st, tl);
  if (rc) return rc;
  const int64_t rows = (int64_t)4 * pl->KX + 3 * pl->K;
  if ((rc = launch_reduce(pl, pl->partial.d(), pl->sp_os.nsplit, KD4, proj, st, -1, nullptr, slice_map(pl, nsl, rows, 0)))) return rc;
  return launch_reduce(pl, pl->partial.d() + (int64_t)pl->sp_os.nsplit * KD4, pl->sp_os.nsplit, KD3, nsl > 1 ? proj : proj + KD4, st, -1,
                       nullptr, slice_map(pl, nsl, rows, (int64_t)4 * pl->KX));
}

// 3. the tail for the snapshots [t0, t0 + nts): linearisation (raw sums of the fields and of the eddy products in the
//    plan's basis), coefficients and zonal means, epilogue.  proj_s: [4 KX + 3 K][nlev][nts], summed over the ranks.
static int os_tail(temx_plan* pl, const double* proj_s, int64_t t0, int64_t nts, double* results, double* zonal, hipStream_t st) {
  int rc;
  set_tail(pl, t0, nts);
  const int64_t Dt = pl->tD;
  const int64_t rows = (int64_t)4 * pl->KX + 3 * pl->K;
  if (proj_s != pl->Ax.d())       // the plan keeps the slice: the tracer's single sweep reuses the projections of v and omega
    HIPCHK(hipMemcpyAsync(pl->Ax.p, proj_s, (size_t)rows * Dt * 8, hipMemcpyDeviceToDevice, st));
  {
    TimedLaunch t2{};
    time_begin(pl, 1, st, t2);
    const size_t lds = os_contract_lds(pl->K, pl->KX, pl->NQ) * 8;
    const double* Pp = pl->Ax.d() + (int64_t)4 * pl->KX * Dt;
    if (pl->osc_lds) {
      OsFields in;
      for (int f = 0; f < 4; ++f) {
        in.A[f] = pl->Ax.d() + (int64_t)f * pl->KX * Dt;
        in.rho[f] = pl->rho.d() + (int64_t)f * pl->KR * pl->D;
      }
      rc = launch_lds<os_contract_kernel<0>, 160 * 1024>(pl->device, dim3((unsigned)((Dt + OSC - 1) / OSC)), dim3(256), lds,
          st, in, Pp, pl->K, pl->KX, pl->KR, pl->NQ, Dt, pl->T.d(), pl->Ginv.d(), pl->G.d(), pl->Gx.d(), pl->gaunt.d(),
          pl->wq2.d(), pl->B4.d(), pl->B3.d(), pl->D, (int)nts, (int)pl->nt, (int)t0);
      if (rc) return rc;
    } else {
      using KD = OsKind<0>;
      const int64_t QD = (int64_t)pl->NQ * Dt;
      OscFieldsIn fin;
      OscPairsIn pin{};
      for (int f = 0; f < 4; ++f) {
        fin.A[f] = pl->Ax.d() + (int64_t)f * pl->KX * Dt;
        fin.rho[f] = pl->rho.d() + (int64_t)f * pl->KR * pl->D;
      }
      for (int k = 0; k < 3; ++k) {
        pin.At_a[k] = pl->osAt.d() + KD::pa(k) * QD; pin.At_b[k] = pl->osAt.d() + KD::pb(k) * QD;
        pin.ab_a[k] = pl->osAb.d() + KD::pa(k) * QD; pin.ab_b[k] = pl->osAb.d() + KD::pb(k) * QD;
        pin.P[k] = Pp + (int64_t)k * pl->K * Dt;
      }
      if ((rc = launch_osc(pl, fin, 4, 4, pl->B4.d(), pl->osAt.d(), pl->osAb.d(), pin, 3, pl->B3.d(), Dt, st))) return rc;
    }
    time_end(pl, 1, st, t2);
  }
  // as after stage 2: coefficients and zonal means of the four fields, then the epilogue
  if ((rc = launch_solve(pl, pl->B4.d(), 4, Dt, pl->C4.d(), pl->zb.d(), st))) return rc;
  if ((rc = tem_stage3_impl(pl, pl->B3.d(), results, zonal, st))) return rc;
  pl->c4_valid = true;
  pl->os_valid = true;            // Ax, rho describe these fields (and these snapshots): the tracer's single sweep may follow
  return TEMX_OK;
}

static int tem_run_os(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, double* results, double* zonal, void* stream) {
  hipStream_t st = S_(stream);
  int rc;
  if ((rc = os_prepass(pl, fp, dtype, pl->Axs.d(), st))) return rc;
  if ((rc = os_sweep(pl, fp, dtype, pl->Axs.d(), 1, pl->Ax.d(), st))) return rc;
  return os_tail(pl, pl->Ax.d(), 0, pl->nt, results, zonal, st);
}

static int tracer_ws(temx_plan* pl);

// Tracers in the single-sweep form: (q, v, omega) -- or (q1, q2, v, omega): one read of v and omega for two tracers --
// read once, no class sums.  The degree-2L projections and the references of v and omega are those the TEM run left in
// the plan (os_valid): the same v and omega must be handed over.  Each q gets its own reference from a pre-pass, is
// projected to degree 2L, q v and q omega to degree L.  The same three steps as the TEM run; for nq tracers:
// Asq[nq][KR][D], projq = nq KX + 2 nq K rows (the q's, then q1 v, q1 omega, q2 v, q2 omega).
static int tracer_os_ws(temx_plan* pl, int nq) {
  const TracerOsWs w = tracer_os_ws_layout(tem_dims(pl), nq, pl->KX, pl->KR, pl->NQ);
  int rc;
  if ((rc = tracer_ws(pl))) return rc;
  if ((rc = pl->Axq.ensure(w.Axq))) return rc;
  if ((rc = pl->osAtq.ensure(w.osAtq))) return rc;
  if ((rc = pl->osAbq.ensure(w.osAbq))) return rc;
  if ((rc = pl->Bqp.ensure(w.Bqp))) return rc;
  return pl->rho_t.ensure(w.rho_t);
}

// fp: (q, v, omega, -) for one tracer, (q1, q2, v, omega) for two
static int tracer_os_prepass(temx_plan* pl, int nq, const FieldPtrs<4>& fp, int dtype, double* Asq, hipStream_t st) {
  int rc;
  const int64_t D = pl->D;
  if ((rc = tracer_os_ws(pl, nq))) return rc;
  pl->tq_valid = false;
  // (the references of v, omega do not matter here: only the projections of the q's are used)
  rc = nq == 2 ? launch_sweep_os<3>(pl, fp, dtype, true, pl->rho0.d(), pl->partial.d(), pl->sp_os_s, st)
               : launch_sweep_os<1>(pl, fp, dtype, true, pl->rho0.d(), pl->partial.d(), pl->sp_os_s, st);
  if (rc) return rc;
  return launch_reduce_rows(pl, pl->partial.d(), pl->sp_os_s.nsplit, (int64_t)nq * pl->KX * D, nq, pl->KX, pl->KR, D, Asq, st);
}

static int tracer_os_sweep(temx_plan* pl, int nq, const FieldPtrs<4>& fp, int dtype, const double* Asq, int nsl, double* projq,
                           hipStream_t st) {
  int rc;
  const int64_t D = pl->D, KXD = (int64_t)pl->KX * D, KD = (int64_t)pl->K * D, KRD = (int64_t)pl->KR * D;
  if ((rc = tracer_os_ws(pl, nq))) return rc;
  pl->tq_valid = false;
  // references: (rho_q, rho_v, rho_omega) / (rho_q1, rho_q2, rho_v, rho_omega), v and omega as the TEM run fitted them
  hipLaunchKernelGGL(os_ref_solve_kernel, dim3((unsigned)((D + 15) / 16), nq), dim3(256), 0, st, Asq, pl->KR, pl->KR, D,
                     pl->Gsinv.d(), pl->rho_t.d());
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(pl->rho_t.d() + nq * KRD, pl->rho.d() + 1 * KRD, (size_t)KRD * 8, hipMemcpyDeviceToDevice, st));         // v
  HIPCHK(hipMemcpyAsync(pl->rho_t.d() + (nq + 1) * KRD, pl->rho.d() + 3 * KRD, (size_t)KRD * 8, hipMemcpyDeviceToDevice, st));   // omega
  rc = nq == 2 ? launch_sweep_os<3>(pl, fp, dtype, false, pl->rho_t.d(), pl->partial.d(), pl->sp_os, st)
               : launch_sweep_os<1>(pl, fp, dtype, false, pl->rho_t.d(), pl->partial.d(), pl->sp_os, st);
  if (rc) return rc;
  const int64_t rows = (int64_t)nq * (pl->KX + 2 * pl->K);
  if ((rc = launch_reduce(pl, pl->partial.d(), pl->sp_os.nsplit, nq * KXD, projq, st, -1, nullptr, slice_map(pl, nsl, rows, 0)))) return rc;
  return launch_reduce(pl, pl->partial.d() + (int64_t)pl->sp_os.nsplit * nq * KXD, pl->sp_os.nsplit, 2 * nq * KD,
                       nsl > 1 ? projq : projq + nq * KXD, st, -1, nullptr, slice_map(pl, nsl, rows, (int64_t)nq * pl->KX));
}

// the tracers' tail for the snapshots the TEM tail worked on (set_tail): projq_s [nq KX + 2 nq K][nlev][tnt]
static int tracer_os_tail(temx_plan* pl, int nq, const double* projq_s, double* const* tres, double* const* tzon, hipStream_t st) {
  int rc;
  const int64_t Dt = pl->tD, KXD = (int64_t)pl->KX * Dt, KDt = (int64_t)pl->K * Dt, KRD = (int64_t)pl->KR * pl->D;
  double* Bq = pl->Bqp.d();                    // [nq][K][Dt]
  double* Bq2 = pl->Bqp.d() + nq * KDt;        // [2 nq][K][Dt]
  if (pl->osc_lds) {
    if (nq != 1) return fail(TEMX_EUNSUPPORTED, "two tracers per sweep need the contraction on the matrix cores (TEMX_OPT_OS_CONTRACT = 0)");
    const size_t lds = os_contract_lds(pl->K, pl->KX, pl->NQ) * 8;
    OsFields in{};
    in.A[0] = projq_s;
    in.A[1] = pl->Ax.d() + 1 * KXD;
    in.A[2] = pl->Ax.d() + 3 * KXD;
    in.rho[0] = pl->rho_t.d();
    in.rho[1] = pl->rho.d() + 1 * KRD;
    in.rho[2] = pl->rho.d() + 3 * KRD;
    rc = launch_lds<os_contract_kernel<1>, 160 * 1024>(pl->device, dim3((unsigned)((Dt + OSC - 1) / OSC)), dim3(256), lds,
        st, in, projq_s + KXD, pl->K, pl->KX, pl->KR, pl->NQ, Dt, pl->T.d(), pl->Ginv.d(), pl->G.d(), pl->Gx.d(),
        pl->gaunt.d(), pl->wq2.d(), Bq, Bq2, pl->D, (int)pl->tnt, (int)pl->nt, (int)pl->tt0);
    if (rc) return rc;
  } else {
    // the q's are synthesised here; v and omega at the nodes are those the TEM tail left in the plan (osAt / osAb)
    const int64_t QD = (int64_t)pl->NQ * Dt;
    OscFieldsIn fin{};
    OscPairsIn pin{};
    const int other[2] = {1, 3};                   // v, omega among the TEM run's four fields
    for (int i = 0; i < nq; ++i) {
      fin.A[i] = projq_s + i * KXD;
      fin.rho[i] = pl->rho_t.d() + i * KRD;
      for (int k = 0; k < 2; ++k) {
        const int p = 2 * i + k;
        pin.At_a[p] = pl->osAtq.d() + i * QD; pin.ab_a[p] = pl->osAbq.d() + i * QD;
        pin.At_b[p] = pl->osAt.d() + other[k] * QD; pin.ab_b[p] = pl->osAb.d() + other[k] * QD;
        pin.P[p] = projq_s + nq * KXD + (int64_t)p * KDt;
      }
    }
    if ((rc = launch_osc(pl, fin, nq, nq, Bq, pl->osAtq.d(), pl->osAbq.d(), pin, 2 * nq, Bq2, Dt, st))) return rc;
  }
  // per tracer: coefficients Ct = (C_q, C_v, C_w) and qb -> tz[0], as the other tracer stage 2 forms leave them
  // (Ct / tz describe the LAST tracer afterwards: temx_tracer_eddy materialises that one)
  const size_t slab = (size_t)pl->K4 * Dt * 8;
  for (int i = 0; i < nq; ++i) {
    if ((rc = launch_solve(pl, Bq + i * KDt, 1, Dt, pl->Ct.d(), pl->tz.d(), st))) return rc;
    HIPCHK(hipMemcpyAsync((char*)pl->Ct.p + slab, (char*)pl->C4.p + slab, slab, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync((char*)pl->Ct.p + 2 * slab, (char*)pl->C4.p + 3 * slab, slab, hipMemcpyDeviceToDevice, st));
    if ((rc = tracer_stage3_impl(pl, Bq2 + 2 * i * KDt, tres[i], tzon ? tzon[i] : nullptr, st))) return rc;
  }
  return TEMX_OK;
}

static FieldPtrs<4> tracer_fields(int nq, const void* const* q, const void* va, const void* wap) {
  return nq == 2 ? four(q[0], q[1], va, wap) : four(q[0], va, wap, nullptr);
}

static int tracer_run_os(temx_plan* pl, int nq, const void* const* q, const void* va, const void* wap, int dtype,
                         double* const* tres, double* const* tzon, void* stream) {
  hipStream_t st = S_(stream);
  int rc;
  if ((rc = tracer_os_ws(pl, nq))) return rc;
  const FieldPtrs<4> fp = tracer_fields(nq, q, va, wap);
  double* Asq = pl->Axq.d() + (int64_t)nq * (pl->KX + 2 * pl->K) * pl->D;
  if ((rc = tracer_os_prepass(pl, nq, fp, dtype, Asq, st))) return rc;
  if ((rc = tracer_os_sweep(pl, nq, fp, dtype, Asq, 1, pl->Axq.d(), st))) return rc;
  return tracer_os_tail(pl, nq, pl->Axq.d(), tres, tzon, st);
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// No exception may cross the C ABI (the callers are ctypes and C): host allocations (std::bad_alloc) and thread
// starts (std::system_error) inside an entry point are the sources.  Every multi-statement entry point is a
// function-try-block ending in TEMX_CATCH.
#define TEMX_CATCH                                                                                     \
  catch (const std::bad_alloc&) { return fail(TEMX_ENOMEM, "out of host memory"); }                   \
  catch (const std::exception& e_) { return fail(TEMX_EINTERNAL, "unexpected C++ exception: %s", e_.what()); } \
  catch (...) { return fail(TEMX_EINTERNAL, "unexpected C++ exception"); }

// ---- missing-value mode: launchers (kernels_miss.hpp) ---------------------------------------------------------
static inline bool miss_mode(const temx_plan* pl) { return pl->opt_missing == 1; }
// latitude-bin form (TEMX_OPT_LAT_BINS): the staged, sharded and single-sweep entry points are refused unless a run
// entry point of this library is what calls them (temx_tracer_run goes through the tracer stages)
static inline bool bin_mode(const temx_plan* pl) { return pl->opt_lat_bins > 0; }
static inline bool bin_refused(const temx_plan* pl) { return bin_mode(pl) && pl->bin_pass == 0; }
struct BinPass {
  temx_plan* pl;
  explicit BinPass(temx_plan* p) : pl(p) { ++pl->bin_pass; }
  ~BinPass() { --pl->bin_pass; }
};
static int bin_refuse(const char* what) {
  return fail(TEMX_EUNSUPPORTED, "%s is not available while latitude bins are in effect (TEMX_OPT_LAT_BINS): the binned form "
              "serves temx_tem_run, temx_project and temx_zonal_mean", what);
}

static inline dim3 bin_sweep_grid(const temx_plan* pl, int64_t D) {
  const int Dw = (int)((D + 63) / 64);
  return dim3((unsigned)(pl->bin_nchunk * ((Dw + 3) / 4)));
}

// pass 1: chunk moments of NF fields
template <int NF>
static int launch_bin_moments(temx_plan* pl, const FieldPtrs<NF>& fp, int dtype, int64_t D, const double* colscale, int sfield,
                              hipStream_t st) {
  const int Dw = (int)((D + 63) / 64);
  if ((int64_t)pl->bin_nchunk * ((Dw + 3) / 4) >= ((int64_t)1 << 31)) return fail(TEMX_EUNSUPPORTED, "latitude bins: too many work units");
  const dim3 grid = bin_sweep_grid(pl, D);
  const int4* ch = static_cast<const int4*>(pl->bin_chunk.p);
  const int* rows = static_cast<const int*>(pl->bin_rows.p);
  return by_dtype(dtype, [&](auto t) {
    return dispatch(BinJValues{}, pl->bin_J, [&](auto j) {
      return launch<bin_moments_kernel<typename decltype(t)::type, NF, decltype(j)::value>>(
          grid, dim3(256), 0, st, fp, D, Dw, ch, rows, pl->bin_s.d(), colscale, sfield, pl->bin_cm.d());
    });
  });
}

static inline double miss_thr(const temx_plan* pl) { return pl->opt_min_cov / 1000.0; }
static inline double miss_omt(const temx_plan* pl) { return 1.0 - std::pow(10.0, -(double)pl->opt_miss_w); }
static int miss_refuse(const char* what) {
  return fail(TEMX_EUNSUPPORTED, "%s is not available in missing-value mode (TEMX_OPT_MISSING = 1): the masked path "
                                 "serves temx_zonal_mean, temx_tem_run and the eddy entry points only", what);
}

// out[NF K + NE][D]: select-projections of the NF fields, then the projection of their common missing indicator
template <int NF>
static int launch_miss_project(temx_plan* pl, const FieldPtrs<NF>& fp, int dtype, int64_t D, const double* colscale,
                               int sfield, double* out, hipStream_t st) {
  return by_dtype(dtype, [&](auto t) {
    const Split sp = choose_split(D, pl->nchunk, pl->num_cu, 4);
    const int64_t R = (int64_t)NF * pl->K + pl->NE;
    if (int rc = pl->partial.ensure((size_t)sp.nsplit * R * D * 8)) return rc;
    const int rc = dispatch(TBValues{}, pl->TB, [&](auto tb) {
      constexpr int TBv = decltype(tb)::value;
      return launch<miss_project_kernel<typename decltype(t)::type, NF, TBv, 2 * TBv>>(
          dim3(sp.grid), dim3(256), 0, st, fp, pl->N, D, pl->K, pl->NE, pl->yblk.d(), pl->stride, pl->eblk.d(), pl->nchunk,
          colscale, sfield, pl->partial.d(), sp.nsplit, sp.ndt);
    });
    return rc ? rc : launch_reduce(pl, pl->partial.d(), sp.nsplit, R * D, out, st);
  });
}

template <int NR>
static int launch_miss_system(temx_plan* pl, const double* Bf, const double* E, int64_t D, double* C, double* Ccov,
                              double* zout, double* cov, hipStream_t st) {
  const int K = pl->K, NQ = pl->NQM, NE = pl->NE;
  const double* t = pl->mtab.d();
  MissTables tb;
  tb.G2 = t;
  tb.Zq = tb.G2 + (size_t)K * K;
  tb.Yq = tb.Zq + (size_t)NQ * K;
  tb.Acov = tb.Yq + (size_t)NQ * NE;
  tb.c1 = tb.Acov + (size_t)K * K;
  tb.Qp = pl->Qp.d();
  hipLaunchKernelGGL(miss_system_kernel<NR>, dim3((unsigned)D), dim3(256), 0, st, Bf, E, K, pl->K4, NE, NQ, pl->M, D, tb,
                     miss_omt(pl), miss_thr(pl), C, Ccov, zout, cov);
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

// the masked eddy sweep: products under the common mask, projected on Q (generic sweep on every grid)
static int launch_miss_eddy(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, hipStream_t st) {
  EddyOut none{};
  return by_dtype(dtype, [&](auto t) {
    return launch_eddy_t<typename decltype(t)::type, 0, 2>(pl, fp, pl->mC.d(), pl->partial.d(), pl->sp_eddy, none, st);
  });
}

static int launch_miss_eddy_native(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, int64_t row0, int64_t nrows,
                                   const EddyOut& eo, hipStream_t st) {
  const int64_t n = nrows * pl->D;
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)pl->num_cu * 16));
  return by_dtype(dtype, [&](auto t) {
    return launch<miss_eddy_native_kernel<typename decltype(t)::type>>(grid, dim3(256), 0, st, fp, row0, nrows, pl->D,
        pl->K, pl->K4, pl->yblk.d(), pl->stride, pl->mC.d(), pl->mCcov.d(), pl->colscale.d(), miss_thr(pl), eo);
  });
}

static int launch_miss_native(temx_plan* pl, const void* A, int dtype, int64_t D, const double* C, const double* Ccov,
                              double* out, hipStream_t st) {
  const int64_t n = pl->N * D;
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)pl->num_cu * 16));
  return by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return launch<miss_native_kernel<T>>(grid, dim3(256), 0, st, static_cast<const T*>(A), pl->N, D, pl->K, pl->yblk.d(),
        pl->stride, C, Ccov, miss_thr(pl), out);
  });
}

// ---- masked tracer run: launchers (kernels_mtracer.hpp, include/temx_mtracer.h) ----------------------------------
// chunks the rows of (q, v, omega) run ahead: 24 ring registers per chunk in fp64.  Two everywhere but at TB = 16 in
// fp64, where 48 + 96 accumulator and 24 staging registers leave room for one inside the 256 of two waves per SIMD
template <typename T, int TB>
constexpr int mtracer_pd() { return (sizeof(T) == 8 && TB == 16) ? 1 : 2; }

// out[K + NE][D]: the select-projection of q under the tracer's mask, then the projection of its missing indicator
static int launch_miss_tracer_project(temx_plan* pl, const FieldPtrs<3>& fp, int dtype, double* out, hipStream_t st) {
  const int64_t D = pl->D;
  return by_dtype(dtype, [&](auto t) {
    const Split sp = choose_split(D, pl->nchunk, 2 * pl->num_cu, 4);
    const int64_t R = (int64_t)pl->K + pl->NE;
    if (int rc = pl->partial.ensure((size_t)sp.nsplit * R * D * 8)) return rc;
    const int rc = dispatch(TBValues{}, pl->TB, [&](auto tb) {
      constexpr int TBv = decltype(tb)::value;
      using T = typename decltype(t)::type;
      return launch<miss_tracer_project_kernel<T, TBv, 2 * TBv, mtracer_pd<T, TBv>()>>(
          dim3(sp.grid), dim3(256), 0, st, fp, pl->N, D, pl->K, pl->NE, pl->yblk.d(), pl->stride, pl->eblk.d(), pl->nchunk,
          pl->partial.d(), sp.nsplit, sp.ndt);
    });
    return rc ? rc : launch_reduce(pl, pl->partial.d(), sp.nsplit, R * D, out, st);
  });
}

// the masked tracer sweep: q'v', q'omega' under the tracer's mask, projected on Q (generic sweep on every grid)
static int launch_miss_tracer_eddy(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, hipStream_t st) {
  EddyOut none{};
  return by_dtype(dtype, [&](auto t) {
    return launch_eddy_t<typename decltype(t)::type, 0, 3>(pl, fp, pl->mtC.d(), pl->partial.d(), pl->sp_eddy, none, st);
  });
}

static int launch_miss_tracer_native(temx_plan* pl, const FieldPtrs<3>& fp, int dtype, const TracerEddyOut& eo,
                                     hipStream_t st) {
  const int64_t n = pl->N * pl->D;
  const dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)pl->num_cu * 16));
  return by_dtype(dtype, [&](auto t) {
    return launch<miss_tracer_native_kernel<typename decltype(t)::type>>(grid, dim3(256), 0, st, fp, pl->N, pl->D, pl->K,
        pl->K4, pl->yblk.d(), pl->stride, pl->mtC.d(), pl->mtCcov.d(), miss_thr(pl), eo);
  });
}

// ---- vertical interpolation: launchers (kernels_vert.hpp, include/temx_vert.h) -----------------------------------
// The tables of a call (hyam, hybm, pt, xt) live in device buffers that are never written again once uploaded, so
// calls on any stream may share them: a call with a set seen before touches no allocator.
struct VertTables {
  int device;
  std::vector<double> host;
  double* dev;
};
static std::mutex g_vert_mu;
static std::vector<VertTables> g_vert_tabs;
constexpr size_t VERT_TABLE_SETS = 16;

static int vert_tables(int device, const std::vector<double>& host, const double** dev) {
  std::lock_guard<std::mutex> lk(g_vert_mu);
  for (const VertTables& e : g_vert_tabs)
    if (e.device == device && e.host == host) {
      *dev = e.dev;
      return TEMX_OK;
    }
  if (g_vert_tabs.size() >= VERT_TABLE_SETS) {   // hipFree waits for the kernels that may still read the oldest set
    (void)hipFree(g_vert_tabs.front().dev);
    g_vert_tabs.erase(g_vert_tabs.begin());
  }
  double* d = nullptr;
  HIPCHK(hipMalloc(&d, host.size() * sizeof(double)));
  hipError_t e = hipMemcpy(d, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return fail(TEMX_EHIP, "upload of the level tables failed: %s", hipGetErrorString(e));
  }
  g_vert_tabs.push_back(VertTables{device, host, d});
  *dev = d;
  return TEMX_OK;
}

template <typename T, int NF, bool HYB>
static int launch_vert(const VertPtrs<NF>& fp, int nf, int64_t ncol, int nlev, int64_t nt, int nplev, const VertTab& tb,
                       double p0, const void* P, int p_f32, int logp, int hold, int map, hipStream_t st) {
  VertSlab sh{};
  size_t lds = 0;
  const bool can_slab = vert_slab_shape(nf, nlev, nt, nplev, sizeof(T), HYB ? 0 : (p_f32 ? 4 : 8), &sh, &lds);
  const bool slab = map == 2 ? can_slab : map == 1 ? false : can_slab && nt * sizeof(T) < 128;
  if (map == 2 && !can_slab) return fail(TEMX_EUNSUPPORTED, "TEMXV_MAP=slab: one column of this shape does not fit the LDS budget");
  if (slab) {
    const int64_t grid = (ncol + sh.cw - 1) / sh.cw;
    if (grid > 0x7fffffff) return fail(TEMX_EUNSUPPORTED, "too many columns for one launch");
    hipLaunchKernelGGL((vert_slab_kernel<T, NF, HYB>), dim3((unsigned)grid), dim3(VERT_THREADS), lds, st, fp, nf, ncol, nlev,
                       (int)nt, nplev, tb, p0, P, p_f32, logp, hold, sh);
  } else {
    const int64_t grid = (ncol * nt + VERT_THREADS - 1) / VERT_THREADS;
    if (grid > 0x7fffffff) return fail(TEMX_EUNSUPPORTED, "too many columns for one launch");
    hipLaunchKernelGGL((vert_time_kernel<T, NF, HYB>), dim3((unsigned)grid), dim3(VERT_THREADS), 0, st, fp, nf, ncol, nlev,
                       nt, nplev, tb, p0, P, p_f32, logp, hold);
  }
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

template <typename T, bool HYB>
static int launch_vert_nf(int nf, const void* const* src, void* const* dst, int64_t ncol, int nlev, int64_t nt, int nplev,
                          const VertTab& tb, double p0, const void* P, int p_f32, int logp, int hold, int map,
                          hipStream_t st) {
  if (nf <= 4) {
    VertPtrs<4> fp{};
    for (int f = 0; f < nf; ++f) fp.src[f] = src[f], fp.dst[f] = dst[f];
    return launch_vert<T, 4, HYB>(fp, nf, ncol, nlev, nt, nplev, tb, p0, P, p_f32, logp, hold, map, st);
  }
  VertPtrs<VERT_NFMAX> fp{};
  for (int f = 0; f < nf; ++f) fp.src[f] = src[f], fp.dst[f] = dst[f];
  return launch_vert<T, VERT_NFMAX, HYB>(fp, nf, ncol, nlev, nt, nplev, tb, p0, P, p_f32, logp, hold, map, st);
}

// ---- the time sum (include/temx_clim.h): one launch for the sources of one dtype ----
template <typename T>
static int launch_time_sum(const ClimPtrs& fp, int nf, int64_t rows, int64_t nt, int accumulate, hipStream_t st) {
  const ClimShape sh = clim_shape(rows, nt, sizeof(T));
  if (sh.nblk >= (int64_t(1) << 32) / CLIM_THREADS)   // HIP takes fewer than 2^32 threads per grid dimension
    return fail(TEMX_EUNSUPPORTED, "too many rows for one launch (%lld workgroups): sum the fields in parts", (long long)sh.nblk);
  if (sh.staged) {
    if ((size_t)sh.rpb * sh.stride * sizeof(T) > (size_t)CLIM_LDS_BYTES || (int64_t)sh.rpb * nt > (int64_t(1) << 30))
      return fail(TEMX_EINTERNAL, "staged rows of the time sum exceed their LDS budget");
    hipLaunchKernelGGL((time_sum_staged_kernel<T>), dim3((unsigned)sh.nblk, (unsigned)nf), dim3(CLIM_THREADS), 0, st, fp, rows,
                       (int)nt, sh, accumulate);
  } else {
    hipLaunchKernelGGL((time_sum_long_kernel<T>), dim3((unsigned)sh.nblk, (unsigned)nf), dim3(CLIM_THREADS), 0, st, fp, rows, nt,
                       accumulate);
  }
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

// ---- the time filter (../include/temx_tfilt.h, kernels_tfilt.hpp): the nf sources of one element type T ----
template <typename T, typename D>
static int launch_tfilt(const TfiltPtrs& fp, int nf, int nb, const double* w, int64_t rows, int64_t nt, int nw, hipStream_t st) {
  const TfiltShape sh = tfilt_shape(rows, nt, nw, nb, sizeof(T), sizeof(D));
  if (sh.grid >= TFILT_GRID_MAX)
    return fail(TEMX_EUNSUPPORTED, "too many rows for one launch (%lld workgroups): filter the fields in parts along ncol",
                (long long)sh.grid);
  if (tfilt_lds_bytes(sh, sizeof(T)) > (size_t)TFILT_LDS_BYTES || sh.TT < TFILT_R || sh.TT % TFILT_R)
    return fail(TEMX_EINTERNAL, "staged rows of the time filter exceed their LDS budget");
  const dim3 grid((unsigned)sh.grid, (unsigned)nf), block(TFILT_THREADS);
  switch (nb) {
    case 1: hipLaunchKernelGGL((tfilt_kernel<T, D, 1>), grid, block, 0, st, fp, w, rows, nt, nw, sh); break;
    case 2: hipLaunchKernelGGL((tfilt_kernel<T, D, 2>), grid, block, 0, st, fp, w, rows, nt, nw, sh); break;
    case 3: hipLaunchKernelGGL((tfilt_kernel<T, D, 3>), grid, block, 0, st, fp, w, rows, nt, nw, sh); break;
    default: hipLaunchKernelGGL((tfilt_kernel<T, D, 4>), grid, block, 0, st, fp, w, rows, nt, nw, sh); break;
  }
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

// ---- the grouped time sum (include/temx_gclim.h, kernels_gclim.hpp) ----
// The table of a record (labels, weights, ng) lives in a device buffer that is never written again once uploaded, as
// the level tables of vert_tables do: every block of a blocked run finds it by content and touches no allocator.
struct GclimTables {
  int device;
  GclimRecord rec;
  unsigned char* dev;
};
static std::mutex g_gclim_mu;
static std::vector<GclimTables> g_gclim_tabs;
constexpr size_t GCLIM_TABLE_SETS = 8;

static int gclim_tables(int device, int ng, int64_t nt_record, const int32_t* label, const double* weight, GclimTab* tb,
                        GclimWindow* win, int64_t t0, int64_t nt) {
  std::lock_guard<std::mutex> lk(g_gclim_mu);
  const std::vector<unsigned char> key = gclim_key(ng, nt_record, label, weight);
  const GclimTables* hit = nullptr;
  for (const GclimTables& e : g_gclim_tabs)
    if (e.device == device && e.rec.key == key) hit = &e;
  if (!hit) {
    if (g_gclim_tabs.size() >= GCLIM_TABLE_SETS) {   // hipFree waits for the kernels that may still read the oldest table
      (void)hipFree(g_gclim_tabs.front().dev);
      g_gclim_tabs.erase(g_gclim_tabs.begin());
    }
    GclimRecord rec = gclim_record(ng, nt_record, label, weight);
    unsigned char* d = nullptr;
    HIPCHK(hipMalloc(&d, rec.image.size()));
    hipError_t e = hipMemcpy(d, rec.image.data(), rec.image.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d);
      return fail(TEMX_EHIP, "upload of the group table failed: %s", hipGetErrorString(e));
    }
    g_gclim_tabs.push_back(GclimTables{device, std::move(rec), d});
    hit = &g_gclim_tabs.back();
  }
  const GclimRecord& r = hit->rec;
  tb->w = reinterpret_cast<const double*>(hit->dev + r.off_w());
  tb->sw = reinterpret_cast<const double*>(hit->dev + r.off_sw());
  tb->lab = reinterpret_cast<const int32_t*>(hit->dev + r.off_lab());
  tb->st = reinterpret_cast<const int32_t*>(hit->dev + r.off_st());
  *win = gclim_window(r, t0, nt);
  return TEMX_OK;
}

// one launch for the sources of one dtype; win.np >= 1
template <typename T>
static int launch_time_sum_groups(const ClimPtrs& fp, int nf, int64_t rows, int64_t nt, int64_t t0, const GclimTab& tb,
                                  const GclimWindow& win, int accumulate, hipStream_t st) {
  const GclimShape gs = gclim_shape(rows, nt, sizeof(T), win.np, win.ng);
  const ClimShape& sh = gs.rows;
  if (gs.nblk >= (int64_t(1) << 32) / CLIM_THREADS)   // HIP takes fewer than 2^32 threads per grid dimension
    return fail(TEMX_EUNSUPPORTED, "too many rows for one launch (%lld workgroups): sum the fields in parts", (long long)gs.nblk);
  const dim3 grid((unsigned)gs.nblk, (unsigned)nf);
  if (sh.staged) {
    if (gs.lds_bytes > (size_t)CLIM_LDS_BYTES || sh.stride < nt || (int64_t)sh.rpb * nt > (int64_t(1) << 30))
      return fail(TEMX_EINTERNAL, "staged rows of the grouped time sum exceed their LDS budget");
    hipLaunchKernelGGL((time_sum_groups_staged_kernel<T>), grid, dim3(CLIM_THREADS), 0, st, fp, rows, (int)nt, (int)t0, sh, tb,
                       win, accumulate);
  } else {
    if (gs.lds_bytes > (size_t)GCLIM_LONG_LDS_BYTES || gs.rpw < 1 || gs.rpw > CLIM_LONG_ROWS)
      return fail(TEMX_EINTERNAL, "long rows of the grouped time sum exceed their LDS budget");
    dispatch(GclimBoundValues{}, gs.bound, [&](auto b) {
      if constexpr (decltype(b)::value == GCLIM_NGMAX)
        hipLaunchKernelGGL((time_sum_groups_long_lds_kernel<T>), grid, dim3(64 * gs.rpw), gs.lds_bytes, st, fp, rows, nt, t0, tb,
                           win, accumulate, gs.rpw);
      else
        hipLaunchKernelGGL((time_sum_groups_long_kernel<T, decltype(b)::value>), grid, dim3(CLIM_THREADS), 0, st, fp, rows, nt,
                           t0, tb, win, accumulate);
      return 0;
    });
  }
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

// ---- the time sum over valid times (include/temx_nclim.h): NFT fields per workgroup, 1 in own-mask mode ----
template <typename T, int NFT>
static int launch_time_sum_valid(const NclimPtrs& fp, int nf, int64_t rows, int64_t nt, int accumulate, hipStream_t st) {
  const NclimShape sh = nclim_shape(rows, nt, sizeof(T), NFT == 1 ? 1 : nf);
  if (sh.nblk >= (int64_t(1) << 32) / NCLIM_THREADS)   // HIP takes fewer than 2^32 threads per grid dimension
    return fail(TEMX_EUNSUPPORTED, "too many rows for one launch (%lld workgroups): sum the fields in parts", (long long)sh.nblk);
  const dim3 grid((unsigned)sh.nblk, NFT == 1 ? (unsigned)nf : 1u);
  if (sh.staged) {
    if ((size_t)(NFT == 1 ? 1 : nf) * sh.rpb * sh.stride * sizeof(T) > (size_t)NCLIM_LDS_BYTES || sh.stride < nt)
      return fail(TEMX_EINTERNAL, "staged rows of the time sum over valid times exceed their LDS budget");
    hipLaunchKernelGGL((time_sum_valid_staged_kernel<T, NFT>), grid, dim3(NCLIM_THREADS), 0, st, fp, nf, rows, (int)nt, sh,
                       accumulate);
  } else {
    hipLaunchKernelGGL((time_sum_valid_long_kernel<T, NFT>), grid, dim3(NCLIM_THREADS), 0, st, fp, nf, rows, nt, accumulate);
  }
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

template <typename T>
static int launch_time_sum_valid_nf(const NclimPtrs& fp, int nf, bool common, int64_t rows, int64_t nt, int accumulate,
                                    hipStream_t st) {
  if (!common) return launch_time_sum_valid<T, 1>(fp, nf, rows, nt, accumulate, st);
  if (nf <= 4) return launch_time_sum_valid<T, 4>(fp, nf, rows, nt, accumulate, st);
  return launch_time_sum_valid<T, NCLIM_NFMAX>(fp, nf, rows, nt, accumulate, st);
}

// ---- the masked grouped time sum (../include/temx_mgclim.h): NFT fields per workgroup, 1 in own-mask mode; win.np >= 1 ----
template <typename T, int NFT>
static int launch_time_sum_groups_valid(int device, const MgclimPtrs& fp, int nf, int64_t rows, int64_t nt, int64_t t0,
                                        const GclimTab& tb, const GclimWindow& win, int accumulate, hipStream_t st) {
  const int nfs = NFT == 1 ? 1 : nf;
  const MgclimShape sh = mgclim_shape(rows, nt, sizeof(T), nfs, win.np);
  if (sh.nblk >= (int64_t(1) << 32) / MGCLIM_THREADS)   // HIP takes fewer than 2^32 threads per grid dimension
    return fail(TEMX_EUNSUPPORTED, "too many rows for one launch (%lld workgroups): sum the fields in parts", (long long)sh.nblk);
  const dim3 grid((unsigned)sh.nblk, NFT == 1 ? (unsigned)nf : 1u);
  if (sh.staged) {
    if (sh.lds_bytes > (size_t)NCLIM_LDS_BYTES || sh.stride < nt || sh.rpb < 1 || sh.rpb > MGCLIM_THREADS)
      return fail(TEMX_EINTERNAL, "staged rows of the masked grouped time sum exceed their LDS budget");
    return launch<time_sum_groups_valid_staged_kernel<T, NFT>>(grid, dim3(MGCLIM_THREADS), 0, st, fp, nf, rows, (int)nt, (int)t0,
                                                               sh.rpb, sh.stride, tb, win, accumulate);
  }
  if (sh.lds_bytes > (size_t)MGCLIM_LONG_LDS_BYTES || sh.rpw < 1 || sh.rpw > NCLIM_LONG_ROWS)
    return fail(TEMX_EINTERNAL, "long rows of the masked grouped time sum exceed their LDS budget");
  return dispatch(GclimBoundValues{}, sh.bound, [&](auto b) {
    if constexpr (decltype(b)::value == GCLIM_NGMAX)
      return launch_lds<time_sum_groups_valid_long_lds_kernel<T, NFT>, MGCLIM_LONG_LDS_BYTES>(
          device, grid, dim3(64 * sh.rpw), sh.lds_bytes, st, fp, nf, rows, nt, t0, tb, win, accumulate, sh.rpw, sh.batch);
    else
      return launch<time_sum_groups_valid_long_kernel<T, NFT, decltype(b)::value>>(grid, dim3(MGCLIM_THREADS), 0, st, fp, nf, rows,
                                                                                   nt, t0, tb, win, accumulate);
  });
}

template <typename T>
static int launch_time_sum_groups_valid_nf(int device, const MgclimPtrs& fp, int nf, bool common, int64_t rows, int64_t nt,
                                           int64_t t0, const GclimTab& tb, const GclimWindow& win, int accumulate,
                                           hipStream_t st) {
  if (!common) return launch_time_sum_groups_valid<T, 1>(device, fp, nf, rows, nt, t0, tb, win, accumulate, st);
  if (nf <= 4) return launch_time_sum_groups_valid<T, 4>(device, fp, nf, rows, nt, t0, tb, win, accumulate, st);
  return launch_time_sum_groups_valid<T, MGCLIM_NFMAX>(device, fp, nf, rows, nt, t0, tb, win, accumulate, st);
}

// ------------------------------------------------------------------------------------------------
// zonal wavenumbers (../include/temx_wave.h, kernels_wave.hpp, wave_tables.hpp)
// ------------------------------------------------------------------------------------------------
struct WaveM {
  int m = 0;
  WaveShape sh;
  DevBuf yblk;      // the deflated basis as 4x4 blocks, sh.gstride blocks per group of 4 rows
  DevBuf pz;        // [M][ndeg] Pbar_l^m at the output latitudes
  DevBuf ginv;      // [Kc][Kc] inverse of Gm = Ym^T Ym, from its Cholesky factor
};

struct temxk_wave {
  temx_plan* pl = nullptr;
  int device = 0;
  std::vector<WaveM> ms;
  int kc_max = 0;
  DevBuf lat, lon, lat_out;     // radians
  DevBuf partial, B, C, flag;   // slabs of the sweep, sums [nf][Kc][D], coefficients [nf][Kc][D], the reduction's own flag
  bool timing = false;          // temxk_wave_timing: events around the projection sweeps of temxk_wave_fluxes
  std::vector<TimedLaunch> timed;
  void drop_events() {
    for (auto& tl : timed) {
      (void)hipEventDestroy(tl.a);
      (void)hipEventDestroy(tl.b);
    }
    timed.clear();
  }
  ~temxk_wave() {
    drop_events();
    for (WaveM& w : ms) {
      w.yblk.release();
      w.pz.release();
      w.ginv.release();
    }
    for (DevBuf* b : {&lat, &lon, &lat_out, &partial, &B, &C, &flag}) b->release();
  }
};

// The wave projection: a workgroup's 4 waves are the 4 fields of one d-tile (NF = 4), or 4 d-tiles of one field (NF = 1).
// Waves per SIMD by the blocks in the accumulators: up to 16 the instantiations of the plan's own sweeps (ProjCfgE /
// ProjCfg1), beyond 16 two -- at three, 25 and 32 blocks spill registers.
template <int NF, int TBv> struct WaveCfg {
  static constexpr int WPS = NF == 1 ? ProjCfg1::WPS : (TBv <= 16 ? ProjCfgE::WPS : 2), DPW = NF == 1 ? 4 : 1;
};
template <int NF>
static Split wave_split(const temx_plan* pl, int64_t D, int tb) {
  const int wps = tb <= 16 ? WaveCfg<NF, 16>::WPS : WaveCfg<NF, 32>::WPS;
  return choose_split(D, pl->nchunk, wps * pl->num_cu, WaveCfg<NF, 16>::DPW);
}

// the deterministic slab sum of launch_reduce, reporting into the wave state's own flag (temxk_wave_status; the plan's is
// plan state)
static int wave_reduce(temxk_wave* w, const double* partial, int nsplit, int64_t stride, int64_t n, double* B, hipStream_t st) {
  return launch_reduce(w->pl, partial, nsplit, n, B, st, stride, nullptr, SliceMap(), static_cast<int*>(w->flag.p));
}

// B[NF][Kc][D] = Ymd^T {fields}: the generic project sweep on the wave basis, one sweep per WAVE_SLICE_TB blocks of columns
template <int NF>
static int wave_sweep(temxk_wave* w, const WaveM& wm, const FieldPtrs<NF>& fp, int dtype, int64_t D, const double* colscale,
                      int sfield, double* B, hipStream_t st) {
  temx_plan* pl = w->pl;
  const WaveShape& sh = wm.sh;
  size_t need = 0;
  for (int sl = 0; sl < sh.nslice; ++sl)
    need = std::max(need, (size_t)wave_split<NF>(pl, D, wave_slice_tb(sh, sl)).nsplit * NF * wave_slice_cols(sh, sl) * D * 8);
  int rc = w->partial.ensure(need);
  if (rc) return rc;
  for (int sl = 0; sl < sh.nslice; ++sl) {
    const int Ks = wave_slice_cols(sh, sl);
    const Split sp = wave_split<NF>(pl, D, wave_slice_tb(sh, sl));
    rc = by_dtype(dtype, [&](auto t) {
      using T = typename decltype(t)::type;
      return dispatch(WaveTBValues{}, wave_slice_tb(sh, sl), [&](auto tb) {
        constexpr int TBv = decltype(tb)::value;
        return launch<project_kernel<T, NF, 1, TBv, 2, WaveCfg<NF, TBv>::WPS>>(
            dim3(sp.grid), dim3(256), 0, st, fp, pl->N, D, Ks, (const double*)wm.yblk.d(), sh.gstride, WAVE_SLICE_TB * sl,
            pl->nchunk, colscale, sfield, w->partial.d(), sp.nsplit, sp.ndt);
      });
    });
    if (rc) return rc;
    if (sh.nslice == 1) return wave_reduce(w, w->partial.d(), sp.nsplit, (int64_t)NF * Ks * D, (int64_t)NF * Ks * D, B, st);
    for (int f = 0; f < NF; ++f)     // the slice's rows of every field, to their place in B
      if ((rc = wave_reduce(w, w->partial.d() + (int64_t)f * Ks * D, sp.nsplit, (int64_t)NF * Ks * D, (int64_t)Ks * D,
                            B + ((int64_t)f * sh.Kc + 4 * WAVE_SLICE_TB * sl) * D, st)))
        return rc;
  }
  return TEMX_OK;
}

static int wave_solve(const WaveM& wm, int nf, int64_t D, const double* B, double* C, hipStream_t st) {
  hipLaunchKernelGGL(wave_solve_kernel, dim3((unsigned)((D + 63) / 64), (unsigned)((wm.sh.Kc + 3) / 4), (unsigned)nf), dim3(256),
                     0, st, B, wm.sh.Kc, D, (const double*)wm.ginv.d(), C);
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

static int wave_ensure(temxk_wave* w, int nf, int64_t D) {
  int rc;
  if ((rc = w->B.ensure((size_t)nf * w->kc_max * D * 8))) return rc;
  return w->C.ensure((size_t)nf * w->kc_max * D * 8);
}

// class form (../include_wavecls/temx_wavecls.h, kernels_wavecls.hpp): what a wavenumber keeps instead of the deflated blocks
struct WaveClsM {
  WaveClsShape sh;
  DevBuf tab;       // [cgroups + 1] class-group tables: the class basis, then -E and -O (wave_class_tables.hpp)
  DevBuf cw;        // [cbatches + CLS_PADB][4][CLS_MB] {cos m lon, sin m lon} of the entries of crow
};

// the class-group tables of one wavenumber from Z = P Ym and the plan's class latitudes
static int wavecls_gather(temx_plan* pl, int m, double pmm_norm, const double* Z, const int* rep, WaveClsM& cm) {
  const int TBS = cm.sh.TBS;
  const size_t bytes = (size_t)(pl->cgroups + 1) * wavecls_group_doubles(TBS) * 8;
  int rc;
  if ((rc = cm.tab.ensure(bytes))) return rc;
  HIPCHK(hipMemset(cm.tab.p, 0, bytes));
  hipLaunchKernelGGL(wavecls_basis_kernel, dim3((unsigned)((pl->ncls + 255) / 256)), dim3(256), 0, nullptr,
                     (const double*)pl->xc.d(), pl->ncls, pl->cls_npad, m, pl->L, pmm_norm, TBS, cm.tab.d());
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(wavecls_defl_kernel, dim3((unsigned)((pl->ncls * cm.sh.Kc + 255) / 256)), dim3(256), 0, nullptr, Z, rep,
                     pl->ncls, cm.sh.ndeg, TBS, cm.tab.d());
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

// one wavenumber: basis, zonal table, Gm and its inverse, deflation by the plan's native zonal-mean operator.  With cm
// (the class form) the deflated blocks are not made: the class tables are gathered from P Ym and the blocks are freed.
static int wave_build_m(temxk_wave* w, WaveM& wm, WaveClsM* cm = nullptr, const int* rep = nullptr) {
  temx_plan* pl = w->pl;
  const WaveShape& sh = wm.sh;
  const int m = wm.m, L = pl->L, Kc = sh.Kc;
  const int64_t N = pl->N, npad = pl->nchunk * 16;
  double r = (2.0 * m + 1.0) / (4.0 * M_PI);
  for (int k = 1; k <= m; ++k) r *= (2.0 * k - 1.0) / (2.0 * k);
  const double pmm_norm = ((m & 1) ? -1.0 : 1.0) * std::sqrt(2.0) * std::sqrt(r);
  int rc;
  if ((rc = wm.yblk.ensure((size_t)npad * sh.kpad * 8))) return rc;
  if ((rc = wm.pz.ensure((size_t)pl->M * sh.ndeg * 8))) return rc;
  if ((rc = wm.ginv.ensure((size_t)Kc * Kc * 8))) return rc;
  DevBuf Ym, Z;                 // row-major basis and its native zonal mean: build time only
  struct Free {
    DevBuf &a, &b;
    ~Free() { a.release(); b.release(); }
  } free_{Ym, Z};
  if ((rc = Ym.ensure((size_t)N * Kc * 8))) return rc;
  if ((rc = Z.ensure((size_t)N * Kc * 8))) return rc;
  hipLaunchKernelGGL(wave_basis_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, nullptr, (const double*)w->lat.d(),
                     (const double*)w->lon.d(), N, npad, m, L, pmm_norm, sh.gstride, Ym.d(), wm.yblk.d());
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(wave_ztable_kernel, dim3((unsigned)((pl->M + 255) / 256)), dim3(256), 0, nullptr,
                     (const double*)w->lat_out.d(), pl->M, m, L, pmm_norm, wm.pz.d());
  HIPCHK(hipGetLastError());
  // Gm = Ym^T Ym: the sweep with the basis itself as the field (D = Kc), before the blocks are deflated
  if ((rc = wave_ensure(w, 1, Kc))) return rc;
  FieldPtrs<1> fp;
  fp.p[0] = Ym.p;
  if ((rc = wave_sweep<1>(w, wm, fp, TEMX_F64, Kc, nullptr, -1, w->B.d(), nullptr))) return rc;
  std::vector<double> G((size_t)Kc * Kc), Gi((size_t)Kc * Kc), F;
  HIPCHK(hipMemcpy(G.data(), w->B.p, G.size() * 8, hipMemcpyDeviceToHost));
  for (double v : G)
    if (!std::isfinite(v)) return fail(TEMX_ERANK, "zonal wavenumber m = %d: the Gram matrix of the basis is not finite", m);
  if (const int piv = wave_cholesky(G.data(), Kc, F))
    return fail(TEMX_ERANK, "zonal wavenumber m = %d: the Gram matrix of its %d basis columns is not positive definite "
                "(pivot %d): the grid does not resolve this wavenumber at L = %d", m, Kc, piv - 1, L);
  wave_inverse_from_factor(F, Kc, Gi.data());
  HIPCHK(hipMemcpy(wm.ginv.p, Gi.data(), Gi.size() * 8, hipMemcpyHostToDevice));
  // Ymd = Ym - P Ym with the plan's own operator (operator workspace of the plan only)
  if ((rc = temx_zonal_mean(pl, Ym.p, TEMX_F64, Kc, Z.d(), 1, nullptr))) return rc;
  if (cm != nullptr) {
    if ((rc = wavecls_gather(pl, m, pmm_norm, Z.d(), rep, *cm))) return rc;
    HIPCHK(hipDeviceSynchronize());
    wm.yblk.release();
    return TEMX_OK;
  }
  hipLaunchKernelGGL(wave_deflate_kernel, dim3((unsigned)((N * Kc + 255) / 256)), dim3(256), 0, nullptr, (const double*)Ym.d(),
                     (const double*)Z.d(), N, Kc, sh.gstride, wm.yblk.d());
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  return TEMX_OK;
}

static int wave_plan_refused(const temx_plan* pl) {
  if (pl->weighted) return fail(TEMX_EUNSUPPORTED, "zonal wavenumbers are not available on a plan in weights mode");
  if (miss_mode(pl)) return fail(TEMX_EUNSUPPORTED, "zonal wavenumbers are not available in missing-value mode (TEMX_OPT_MISSING = 1)");
  if (bin_mode(pl)) return fail(TEMX_EUNSUPPORTED, "zonal wavenumbers are not available while latitude bins are in effect (TEMX_OPT_LAT_BINS)");
  if (pl->ext_G)
    return fail(TEMX_EUNSUPPORTED, "zonal wavenumbers are not available on a plan finalised with a Gram matrix from outside "
                "(an ncol-sharded job): the fit runs over all columns of the grid");
  return TEMX_OK;
}

// ---- the class form of the fit (../include_wavecls/temx_wavecls.h) ----
// What the two forms share -- latitudes, Pz, Gm^-1, the workspace, the flag, the solve and the flux and parts kernels -- is
// a generic state whose deflated blocks are never kept.
struct temxz_wave {
  temxk_wave g;
  std::vector<WaveClsM> cm;     // per wavenumber, aligned with g.ms
  ~temxz_wave() {
    for (WaveClsM& c : cm) {
      c.tab.release();
      c.cw.release();
    }
  }
};

static int wavecls_plan_refused(const temx_plan* pl) {
  if (int rc = wave_plan_refused(pl)) return rc;
  if ((!pl->cls && !pl->lcls) || pl->h_crow.empty())
    return fail(TEMX_EUNSUPPORTED, "the class form of the wave fit needs a plan with latitude classes (columns that share "
                "latitudes); this plan has none: use the generic form");
  return TEMX_OK;
}

// one field per wave: the four fields of a d-tile (NF = 4) or four d-tiles of one field (NF = 1) per workgroup
template <int NF>
static Split wavecls_split(const temx_plan* pl, int64_t D) {
  return choose_split(D, std::max<int64_t>(1, pl->cbatches / 4), WAVECLS_WPS * pl->num_cu, NF == 1 ? 4 : 1, TEMX_CLS_MINCHUNK);
}
// X batches a wave holds (PD - 1 in flight): a batch of fp32 carries half the bytes
template <typename T> constexpr int wavecls_pd() { return sizeof(T) == 4 ? 3 : 2; }

// B[NF][Kc][D] = (Ym - P Ym)^T {fields} by the class sweep and the deterministic slab sum
template <int NF>
static int wavecls_sweep(temxz_wave* z, size_t mi, const FieldPtrs<NF>& fp, int dtype, int64_t D, const double* colscale,
                         int sfield, double* B, hipStream_t st) {
  temxk_wave* w = &z->g;
  temx_plan* pl = w->pl;
  const WaveClsM& cm = z->cm[mi];
  const Split sp = wavecls_split<NF>(pl, D);
  const int64_t n = (int64_t)NF * cm.sh.Kc * D;
  int rc = w->partial.ensure((size_t)sp.nsplit * (size_t)n * 8);
  if (rc) return rc;
  const int2* cuts = nullptr;
  if ((rc = class_cuts_dev(pl, sp.nsplit, &cuts))) return rc;
  rc = by_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatch(WaveClsTBSValues{}, cm.sh.TBS, [&](auto tbs) {
      return launch<wavecls_project_kernel<T, NF, decltype(tbs)::value, WAVECLS_WPS, wavecls_pd<T>()>>(
          dim3(sp.grid), dim3(256), 0, st, fp, D, cm.sh.ndeg, (const double*)cm.tab.d(), static_cast<const int4*>(pl->crow.p),
          static_cast<const double2*>(cm.cw.p), cuts, colscale, sfield, w->partial.d(), sp.nsplit, sp.ndt);
    });
  });
  if (rc) return rc;
  return wave_reduce(w, w->partial.d(), sp.nsplit, n, n, B, st);
}

extern "C" {

int temx_version(void) { return 402; }

const char* temx_last_error(void) { return g_err.c_str(); }

int temx_device_count(void) try {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
} TEMX_CATCH

void temx_plan_destroy(temx_plan* pl) {
  if (!pl) return;
  (void)hipSetDevice(pl->device);
  DevBuf* bufs[] = {&pl->x, &pl->Y0, &pl->yblk, &pl->yblk_w, &pl->Y0p, &pl->G, &pl->Ginv, &pl->norm,
                    &pl->flag, &pl->p, &pl->pg, &pl->lg, &pl->coslat, &pl->fcor, &pl->colscale,
                    &pl->B4, &pl->B3, &pl->C4, &pl->zb, &pl->partial, &pl->opB, &pl->opC,
                    &pl->Bq, &pl->Bq2, &pl->Ct, &pl->tz, &pl->rows, &pl->ysym, &pl->Bs, &pl->XB, &pl->P3};
  for (DevBuf* b : bufs) b->release();
  pl->crow.release();
  pl->ycls.release();
  pl->csum.release();
  pl->ccnt.release();
  pl->Pq.release();
  pl->csq.release();
  pl->Pq2.release();
  pl->ycls_l.release();
  pl->pbuf.release();
  pl->gblk.release();
  pl->ypblk.release();
  for (DevBuf* b : {&pl->T, &pl->Qp, &pl->GinvA, &pl->G2, &pl->xo, &pl->xc, &pl->ycx, &pl->ycx_s, &pl->crow_s, &pl->side_crow[0][0], &pl->side_crow[0][1], &pl->side_crow[1][0], &pl->side_crow[1][1],
                    &pl->side_gfirst[0][0], &pl->side_gfirst[0][1], &pl->side_gfirst[1][0], &pl->side_gfirst[1][1], &pl->rho,
                    &pl->rho0, &pl->gaunt, &pl->wq2, &pl->Axq, &pl->rho_t, &pl->Gx, &pl->Gsinv, &pl->Ax, &pl->Axs, &pl->oscblk, &pl->osAt, &pl->osAb, &pl->osAtq, &pl->osAbq, &pl->Bqp})
    b->release();
  for (DevBuf* b : {&pl->eblk, &pl->mtab, &pl->mB, &pl->mC, &pl->mCcov, &pl->mcov, &pl->mZ}) b->release();
  for (DevBuf* b : {&pl->mtB, &pl->mtB2, &pl->mtC, &pl->mtCcov, &pl->mtz}) b->release();
  for (DevBuf* b : {&pl->bin_a, &pl->bin_chunk, &pl->bin_c0, &pl->bin_rows, &pl->bin_s, &pl->bin_T, &pl->bin_cm, &pl->bin_z, &pl->bin_cy}) b->release();
  for (auto& kv : pl->csplits_s) kv.second.release();
  for (auto& kv : pl->csplits) kv.second.release();
  for (int w = 0; w < 2; ++w)
    for (auto& tl : pl->timed[w]) {
      (void)hipEventDestroy(tl.a);
      (void)hipEventDestroy(tl.b);
    }
  delete pl;
}

// native rows: canonical [N][K] copy (Y0c, may be null) and the 4x4 blocks of the sweeps (yblk, may be null);
// T: null for Y0 itself, or the device copy of R^-1 for the rows of Q = Y0 R^-1
static int build_basis(temx_plan* pl, const double* rowscale_dev, const double* T, double* Y0c, double* yblk) {
  const int64_t npad = pl->nchunk * 16;
  return by_basis_rows(pl->K, [&](auto r) {
    return launch<basis_kernel<decltype(r)::value>>(dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, nullptr, pl->x.d(),
        pl->N, npad, pl->K, pl->stride, pl->norm.d(), rowscale_dev, T, Y0c, yblk);
  });
}

// rows at the output latitudes: canonical [M][K] into `dst`; for K <= 64 also the blocked copy of Qp
static int build_out_basis(temx_plan* pl, const double* T, double* dst, bool blocks) {
  const int64_t mch = (pl->M + 15) / 16;
  const int rc = by_basis_rows(pl->K, [&](auto r) {
    return launch<basis_kernel<decltype(r)::value>>(dim3((unsigned)((mch * 16 + 255) / 256)), dim3(256), 0, nullptr,
        pl->xo.d(), (int64_t)pl->M, mch * 16, pl->K, pl->stride, pl->norm.d(), (const double*)nullptr, T, dst,
        (double*)nullptr);
  });
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  if (blocks && pl->K <= 64) {   // blocked copy for solve_mfma_kernel
    std::vector<double> yp((size_t)pl->M * pl->K);
    HIPCHK(hipMemcpy(yp.data(), dst, yp.size() * 8, hipMemcpyDeviceToHost));
    return upload(pl->ypblk, pack_blocks4(yp.data(), pl->M, pl->K, pl->TB));
  }
  return TEMX_OK;
}

// basis rows at the class latitudes (kernels_cls.hpp): ycls, or the 64-harmonic slices ycls_l
static int build_cls_basis(temx_plan* pl, const double* T) {
  const unsigned nb = (unsigned)((pl->cls_npad + 255) / 256);
  return by_basis_rows(pl->K, [&](auto r) {
    constexpr int R = decltype(r)::value;
    if (pl->lcls) {
      for (int sl = 0; sl < pl->nslice; ++sl)
        hipLaunchKernelGGL(cls_basis_slice_kernel<R>, dim3(nb), dim3(256), 0, 0, pl->xc.d(), pl->ncls, pl->cls_npad, pl->K,
            64 * sl, pl->norm.d(), T, pl->ycls_l.d() + sl * pl->ycls_lstride);
    } else if (pl->cls) {
      hipLaunchKernelGGL(cls_basis_kernel<R>, dim3(nb), dim3(256), 0, 0, pl->xc.d(), pl->ncls, pl->cls_npad, pl->K, pl->TBS,
                         pl->norm.d(), T, pl->ycls.d());
    }
    HIPCHK(hipGetLastError());
    return (int)TEMX_OK;
  });
}

static int build_sym_basis(temx_plan* pl, const double* T) {
  if (!pl->sym) return TEMX_OK;
  const int64_t n4 = pl->npg_alloc * 4;
  return by_basis_rows(pl->K, [&](auto r) {
    return launch<sym_basis_kernel<decltype(r)::value>>(dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, nullptr, pl->x.d(),
                                                        static_cast<const int*>(pl->rows.p), pl->npair, n4, pl->K, pl->TBS,
                                                        pl->norm.d(), T, pl->ysym.d());
  });
}

// every projection / reconstruction operand of the plan in the basis T (null: Y0 itself)
static int build_all_bases(temx_plan* pl, const double* T) {
  int rc;
  if ((rc = build_basis(pl, nullptr, T, nullptr, pl->yblk.d()))) return rc;
  if ((rc = build_cls_basis(pl, T))) return rc;
  if ((rc = build_sym_basis(pl, T))) return rc;
  if ((rc = build_out_basis(pl, T, pl->Qp.d(), true))) return rc;
  HIPCHK(hipDeviceSynchronize());
  return TEMX_OK;
}

int temx_plan_create(temx_plan** out, int device, int64_t ncol, int L, int M,
                     const double* lat_deg_host, const double* lat_out_deg_host, int flags) try {
  if (!out || !lat_deg_host || !lat_out_deg_host) return fail(TEMX_EINVAL, "null argument");
  *out = nullptr;
  if (ncol < 1 || M < 1 || L < 0) return fail(TEMX_EINVAL, "ncol, M must be >= 1 and L >= 0");
  if (L > 511) return fail(TEMX_EUNSUPPORTED, "L = %d: this version supports L <= 511", L);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(TEMX_EHIP, "device %d not available (%d visible)", device, ndev);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(TEMX_EUNSUPPORTED, "libtemx is built for gfx950 (MI355X); device is %s", prop.gcnArchName);

  temx_plan* pl = new temx_plan();
  pl->device = device;
  pl->no_qr = (flags & TEMX_NO_QR) != 0;
  const double tol_dflt = (flags & TEMX_LAT_TOL_F32) ? 1e-8 : 1e-11;   // degrees; see sym_tol_deg
  pl->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  pl->N = ncol;
  pl->nchunk = (ncol + 15) / 16;
  pl->L = L;
  pl->K = L + 1;
  // l-blocks of 4 harmonics per row; the sweeps are instantiated for TB in {4, 8, 13, 16}
  pl->TB = pl->K <= 16 ? 4 : (pl->K <= 32 ? 8 : (pl->K <= 52 ? 13 : 16));
  pl->stride = pl->TB;
  if (pl->K > 64) {   // several slices of 64 harmonics: sliced sweeps instead of the fused ones
    pl->large = true;
    pl->nslice = (pl->K + 63) / 64;
    pl->stride = 16 * pl->nslice;
  }
  pl->K4 = 4 * pl->stride;
  pl->M = M;
  pl->lat_out_deg.assign(lat_out_deg_host, lat_out_deg_host + M);
  pl->h_lat.assign(lat_deg_host, lat_deg_host + ncol);
  int rc = TEMX_OK;
  auto bail = [&](int code) {
    temx_plan_destroy(pl);
    return code;
  };

  // x = cos(colat), colat = deg2rad(90 - lat)   (sph_zonal_mean.py:361)
  const double d2r = M_PI / 180.0;
  std::vector<double> xs((size_t)std::max<int64_t>(ncol, M));
  for (int64_t i = 0; i < ncol; ++i) xs[i] = std::cos((90.0 - lat_deg_host[i]) * d2r);
  if ((rc = upload(pl->x, xs.data(), (size_t)ncol * 8))) return bail(rc);
  std::vector<double> norm((size_t)std::max(64, pl->K4), 0.0);
  for (int l = 0; l < pl->K; ++l) norm[l] = std::sqrt((2.0 * l + 1.0) / (4.0 * M_PI));
  if ((rc = upload(pl->norm, norm.data(), norm.size() * 8))) return bail(rc);
  const int zero[2] = {0, 0};          // [0] non-finite input seen, [1] the single sweep's hand-over status
  if ((rc = upload(pl->flag, zero, sizeof(zero)))) return bail(rc);

  if ((rc = pl->Y0.ensure((size_t)ncol * pl->K * 8))) return bail(rc);
  // one extra chunk of blocks: the sweeps prefetch A operands one group / step ahead
  if ((rc = pl->yblk.ensure((size_t)(pl->nchunk + 1) * 4 * pl->stride * 16 * 8))) return bail(rc);
  if (hipMemset(pl->yblk.p, 0, pl->yblk.bytes) != hipSuccess) return bail(fail(TEMX_EHIP, "hipMemset of the Y0 blocks failed"));
  if ((rc = build_basis(pl, nullptr, nullptr, pl->Y0.d(), pl->yblk.d()))) return bail(rc);

  // Y0p on the output latitudes (sph_zonal_mean.py:367-370): same kernel, canonical copies only (Y0p the
  // attribute, Qp the device operand -- equal until temx_plan_finalize changes the basis)
  for (int m = 0; m < M; ++m) xs[m] = std::cos((90.0 - lat_out_deg_host[m]) * d2r);
  if ((rc = upload(pl->xo, xs.data(), (size_t)M * 8))) return bail(rc);
  if ((rc = pl->Y0p.ensure((size_t)M * pl->K * 8))) return bail(rc);
  if ((rc = pl->Qp.ensure((size_t)M * pl->K * 8))) return bail(rc);
  if ((rc = build_out_basis(pl, nullptr, pl->Y0p.d(), false))) return bail(rc);
  if ((rc = build_out_basis(pl, nullptr, pl->Qp.d(), true))) return bail(rc);

  // local Gram G = Y0^T Y0 through the projection sweep itself (A = Y0, D = K)
  {
    if ((rc = pl->G.ensure((size_t)pl->K * pl->K * 8))) return bail(rc);
    if ((rc = pl->Ginv.ensure((size_t)pl->K * pl->K * 8))) return bail(rc);
    Split sp = choose_split(pl->K, pl->nchunk, 2 * pl->num_cu);
    if ((rc = pl->partial.ensure((size_t)sp.nsplit * std::min(pl->K, 64) * pl->K * 8))) return bail(rc);
    FieldPtrs<1> fp;
    fp.p[0] = pl->Y0.p;
    if ((rc = project_all<1>(pl, fp, TEMX_F64, pl->K, nullptr, -1, sp, pl->G.d(), 0))) return bail(rc);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return bail(fail(TEMX_EHIP, "gram kernel failed: %s", hipGetErrorString(e)));
  }
  {   // blocks of 4 even (or odd) harmonics in the paired / class sweeps
    const int nhalf = (pl->K + 1) / 2;                         // even harmonics (>= odd ones)
    const int tbs = (nhalf + 3) / 4;
    pl->TBS = tbs <= 2 ? 2 : (tbs <= 4 ? 4 : (tbs <= 7 ? 7 : 8));
  }
  // latitude classes (kernels_cls.hpp): columns that share |lat| share a basis row -- the MFMA work
  // is per class and the sweeps become HBM streams (cubed-sphere: 16 columns per class)
  {
    const char* e0 = getenv("TEMX_NO_SYM");
    const char* e1 = getenv("TEMX_NO_CLS");
    ClassTables ct;
    if ((!pl->large || pl->K <= 256) && !(flags & (TEMX_NO_SYMMETRY | TEMX_NO_CLASSES)) && !(e0 && e0[0] == '1') &&
        !(e1 && e1[0] == '1') &&
        build_classes(lat_deg_host, ncol, ct, sym_tol_deg(tol_dflt), (flags & TEMX_LAT_TOL_F32) ? (size_t)TEMX_F32_SIDE_CAP : 0, TEMX_F32_SIDE_KEEP)) {
      if ((rc = upload(pl->crow, ct.crow.data(), ct.crow.size() * sizeof(int)))) return bail(rc);

      if ((rc = upload(pl->ccnt, ct.cnt.data(), ct.cnt.size() * 8))) return bail(rc);
      if ((rc = upload(pl->xc, ct.xc.data(), ct.xc.size() * 8))) return bail(rc);
      pl->h_xc = ct.xc;
      pl->h_cnt = ct.cnt;
      pl->h_crow = ct.crow;
      if (const char* dp = getenv("TEMX_DUMP_CROW")) {     // development: the row table as tools/sweep_lab.hip reads it (LAB_CROW)
        if (FILE* fh = fopen(dp, "wb")) {
          const int32_t hdr[2] = {(int32_t)ct.ngroups, (int32_t)ct.crow.size()};
          fwrite(hdr, 4, 2, fh);
          fwrite(ct.gbatch0.data(), 4, (size_t)ct.ngroups + 1, fh);
          fwrite(ct.crow.data(), 4, ct.crow.size(), fh);
          fclose(fh);
        }
      }
      pl->cls_npad = (ct.ngroups + 1) * 4;
      pl->gbatch0 = std::move(ct.gbatch0);
      pl->cgroups = ct.ngroups;
      pl->cbatches = ct.nbatch;
      pl->ncls = ct.ncls;
      pl->cls_max_side = ct.max_side;
      if (pl->large) {   // class sums first, sliced basis at the class latitudes (kernels_cls.hpp)
        pl->ycls_lstride = (ct.ngroups + 1) * 256;
        if ((rc = pl->ycls_l.ensure((size_t)pl->nslice * pl->ycls_lstride * 8))) return bail(rc);
        pl->lcls = true;
      } else {
        if ((rc = pl->ycls.ensure((size_t)(ct.ngroups + 1) * 2 * pl->TBS * 16 * 8))) return bail(rc);
        pl->cls = true;
      }
      if ((rc = build_cls_basis(pl, nullptr))) return bail(rc);
      {
        hipError_t e2 = hipDeviceSynchronize();
        if (e2 != hipSuccess) return bail(fail(TEMX_EHIP, "class basis kernel failed: %s", hipGetErrorString(e2)));
      }
    }
  }
  // mirror pairing (kernels_sym.hpp): ~46 % fewer MFMAs on equatorially symmetric grids
  if (!pl->cls) {
    const char* e = getenv("TEMX_NO_SYM");
    std::vector<int> rN, rS;
    if (!pl->large && !(flags & TEMX_NO_SYMMETRY) && !(e && e[0] == '1') && find_mirror_pairs(lat_deg_host, ncol, rN, rS, sym_tol_deg(tol_dflt))) {
      pl->npair = (int64_t)rN.size();
      pl->npg = (pl->npair + 3) / 4;
      pl->npg_alloc = ((pl->npg + SYM_PROJ_CH - 1) / SYM_PROJ_CH + 1) * SYM_PROJ_CH;   // whole chunks + 1 chunk
      const int64_t n4 = pl->npg_alloc * 4;
      std::vector<int> rows((size_t)2 * n4, 0);
      for (int64_t k = 0; k < n4; ++k) rows[(size_t)n4 + k] = -1;
      for (int64_t k = 0; k < pl->npair; ++k) {
        rows[(size_t)k] = rN[(size_t)k];
        rows[(size_t)n4 + k] = rS[(size_t)k];
      }
      if ((rc = upload(pl->rows, rows.data(), rows.size() * sizeof(int)))) return bail(rc);
      if ((rc = pl->ysym.ensure((size_t)pl->npg_alloc * 2 * pl->TBS * 16 * 8))) return bail(rc);
      pl->sym = true;
      if ((rc = build_sym_basis(pl, nullptr))) return bail(rc);
      hipError_t e2 = hipDeviceSynchronize();
      if (e2 != hipSuccess) return bail(fail(TEMX_EHIP, "sym basis kernel failed: %s", hipGetErrorString(e2)));
    }
  }
  if (!(flags & TEMX_DEFER_FINALIZE)) {
    if ((rc = temx_plan_finalize(pl, nullptr))) return bail(rc);
  }
  *out = pl;
  return TEMX_OK;
} TEMX_CATCH

int temx_plan_is_paired(const temx_plan* pl) { return pl && (pl->sym || pl->cls) ? 1 : 0; }

int temx_plan_sweep_mode(const temx_plan* pl) try {
  return !pl ? -1 : ((pl->cls || (pl->lcls && pl->lone)) ? 2 : (pl->sym ? 1 : 0));
} TEMX_CATCH

int temx_plan_one_pass(const temx_plan* pl) try {
  return pl && ((pl->cls && pl->onepass) || (pl->lcls && pl->lone)) ? 1 : 0;
} TEMX_CATCH

int temx_plan_single_sweep(const temx_plan* pl) { return pl && pl->os_on ? 1 : 0; }

// G2 (device) = Q^T Q over this plan's rows, through the projection sweep (A = Q, D = K)
static int gram_of_q(temx_plan* pl) {
  DevBuf Qc;
  int rc = Qc.ensure((size_t)pl->N * pl->K * 8);
  if (rc) return rc;
  if ((rc = pl->G2.ensure((size_t)pl->K * pl->K * 8)) == TEMX_OK &&
      (rc = build_basis(pl, nullptr, pl->T.d(), Qc.d(), nullptr)) == TEMX_OK) {
    Split sp = choose_split(pl->K, pl->nchunk, 2 * pl->num_cu);
    FieldPtrs<1> fp;
    fp.p[0] = Qc.p;
    rc = project_all<1>(pl, fp, TEMX_F64, pl->K, nullptr, -1, sp, pl->G2.d(), 0);
  }
  hipError_t e = hipDeviceSynchronize();
  Qc.release();
  if (rc) return rc;
  if (e != hipSuccess) return fail(TEMX_EHIP, "gram kernel failed: %s", hipGetErrorString(e));
  return TEMX_OK;
}

// Replaces lstsq(Y0, I_N) (sph_zonal_mean.py:389).  The Gram matrix G = Y0^T Y0 squares the condition
// number of Y0, and multiplying by an explicit G^-1 squares it once more (measured on a random grid with
// cond(G) = 5.9e3: 1.4e-9 from the reference's SVD solution, profiles/r02_fuzz_seed_887.log).  So the plan
// re-orthogonalises (Cholesky-QR2): R from the Cholesky factorisation of G (long double), every basis block
// of the sweeps rebuilt for Q = Y0 R^-1 -- a row of Q still depends on latitude only, and with an
// equatorially symmetric grid R does not mix even and odd harmonics, so the class / paired sweeps keep
// working -- then the Gram matrix of Q (the identity up to cond(G) eps) factorised once more
// (temx_plan_refine).  The sweeps project on Q, the K x K "solve" multiplies by (Q^T Q)^-1 ~ I, and Qp = Y0p
// R^-1 takes the coefficients to the output latitudes: errors of order cond(Y0) eps.  Attributes (Y0, Y0p,
// Y0inv = G^-1 Y0^T) are unchanged.  TEMX_NO_QR=1 keeps the plain normal equations (A/B runs).
int temx_plan_finalize(temx_plan* pl, const double* G_host) try {
  if (!pl) return fail(TEMX_EINVAL, "null plan");
  HIPCHK(hipSetDevice(pl->device));
  const int K = pl->K;
  std::vector<double> G((size_t)K * K), Gi((size_t)K * K);
  if (G_host) {
    if (pl->h_G_own.empty()) {    // TEMX_MAT_GRAM stays this rank's own sums (a second runner all-reduces them again)
      pl->h_G_own.resize((size_t)K * K);
      HIPCHK(hipMemcpy(pl->h_G_own.data(), pl->G.p, G.size() * 8, hipMemcpyDeviceToHost));
    }
    std::copy(G_host, G_host + (size_t)K * K, G.begin());
    HIPCHK(hipMemcpy(pl->G.p, G.data(), G.size() * 8, hipMemcpyHostToDevice));
  } else {
    HIPCHK(hipMemcpy(G.data(), pl->G.p, G.size() * 8, hipMemcpyDeviceToHost));
  }
  for (double v : G)
    if (!std::isfinite(v)) return fail(TEMX_EINVAL, "Gram matrix is not finite (NaN latitudes?)");
  pl->h_G = G;                    // (as on the device: before the odd entries are cleared)
  if (pl->qbasis) {               // finalised before: back to the Y0 basis the Gram matrix refers to
    if (int rcb = build_all_bases(pl, nullptr)) return rcb;
    pl->qbasis = false;
  }
  // On an equatorially symmetric grid G[l][m] vanishes for l + m odd; the entries that rounding left
  // there are cleared, so that R (and Q) keep the parity the class / paired sweeps rely on.
  const bool parity_paths = pl->sym || pl->cls || pl->lcls;
  double odd_max = 0.0, diag_max = 0.0;
  for (int i = 0; i < K; ++i) {
    diag_max = std::max(diag_max, std::fabs(G[(size_t)i * K + i]));
    for (int j = 0; j < K; ++j)
      if ((i + j) & 1) odd_max = std::max(odd_max, std::fabs(G[(size_t)i * K + j]));
  }
  const bool checker = odd_max <= 1e-10 * diag_max;
  pl->ext_G = G_host != nullptr;
  pl->g_checker = checker && (G_host != nullptr || parity_paths);
  if (pl->g_checker)
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j)
        if ((i + j) & 1) G[(size_t)i * K + j] = 0.0;
  std::vector<long double> Li;
  const bool spd = spd_factor(G.data(), K, Li) == 0;
  if (!spd) {
    // rank-deficient Y0: pseudo-inverse, like the reference's lstsq (sph_zonal_mean.py:389)
    int rank = 0;
    if (sym_pinv(G.data(), K, Gi.data(), &rank) != 0 || rank == 0)
      return fail(TEMX_ERANK, "Y0^T Y0 has no positive eigenvalue (N=%lld, K=%d)", (long long)pl->N, K);
    pl->rank = rank;
  } else {
    inverse_from_factor(Li, K, Gi.data());
    pl->rank = K;
  }
  if (int rca = upload(pl->GinvA, Gi.data(), Gi.size() * 8)) return rca;
  const char* eq = getenv("TEMX_NO_QR");
  const bool no_qr = eq ? eq[0] == '1' : pl->no_qr;
  // Q = Y0 R^-1 keeps the parity of the harmonics only when G is a checkerboard (an equatorially symmetric grid);
  // the class / paired sweeps need that.  With an external G (ncol-sharded: the all-reduced one) every rank must
  // make the SAME choice whatever sweeps its own block of columns runs, so the choice depends on G alone there.
  const bool want_q = spd && !no_qr && (G_host ? checker : (!parity_paths || checker));
  if (want_q) {
    std::vector<double> T((size_t)K * K, 0.0), I((size_t)K * K, 0.0);
    for (int l = 0; l < K; ++l) {
      I[(size_t)l * K + l] = 1.0;
      for (int j = l; j < K; ++j) T[(size_t)l * K + j] = (double)Li[(size_t)j * K + l];   // R^-1 = (L^-1)^T
    }
    if (int rct = upload(pl->T, T.data(), T.size() * 8)) return rct;
    pl->h_T = T;
    if (int rcb = build_all_bases(pl, pl->T.d())) return rcb;
    pl->qbasis = true;
    if (int rcg = set_ginv(pl, I.data())) return rcg;      // until temx_plan_refine
  } else {
    if (int rcg = set_ginv(pl, Gi.data())) return rcg;
  }
  int zero = 0;
  HIPCHK(hipMemcpy(pl->flag.p, &zero, sizeof(int), hipMemcpyHostToDevice));
  pl->finalized = true;
  pl->op_valid = pl->c4_valid = pl->xb_valid = pl->tq_valid = false;   // sums / coefficients of another basis
  pl->miss_built = pl->miss_valid = false;
  pl->bin_built = 0;
  // one process owns all the rows: second pass of the re-orthogonalisation with its own Gram matrix of Q
  if (want_q && !G_host) return temx_plan_refine(pl, nullptr);
  return TEMX_OK;
} TEMX_CATCH

int temx_plan_refine(temx_plan* pl, const double* G2_host) try {
  if (!pl) return fail(TEMX_EINVAL, "null plan");
  if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
  if (!pl->qbasis) return TEMX_OK;                 // normal equations / pseudo-inverse / weights: nothing to refine
  HIPCHK(hipSetDevice(pl->device));
  const int K = pl->K;
  std::vector<double> G2((size_t)K * K), Gi((size_t)K * K);
  if (G2_host) {
    std::copy(G2_host, G2_host + (size_t)K * K, G2.begin());
  } else {
    if (int rc = gram_of_q(pl)) return rc;
    HIPCHK(hipMemcpy(G2.data(), pl->G2.p, G2.size() * 8, hipMemcpyDeviceToHost));
  }
  for (double v : G2)
    if (!std::isfinite(v)) return fail(TEMX_EINVAL, "second Gram matrix is not finite");
  if (pl->g_checker)                               // same parity argument as in temx_plan_finalize
    for (int i = 0; i < K; ++i)
      for (int j = 0; j < K; ++j)
        if ((i + j) & 1) G2[(size_t)i * K + j] = 0.0;
  std::vector<long double> Li;
  if (spd_factor(G2.data(), K, Li) != 0) return TEMX_OK;   // (cannot happen for Q^T Q ~ I; keep the identity)
  inverse_from_factor(Li, K, Gi.data());
  pl->miss_built = pl->miss_valid = false;
  pl->bin_built = 0;
  return set_ginv(pl, Gi.data());
} TEMX_CATCH

int temx_plan_set_weights(temx_plan* pl, const double* w_host) try {
  if (!pl || !w_host) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  // Y0inv = Y0^T diag(4 pi w)  (sph_zonal_mean.py:181, 385): scale the projection operand rows,
  // and make the "Gram inverse" the identity.
  std::vector<double> w((size_t)pl->N);
  for (int64_t i = 0; i < pl->N; ++i) w[i] = w_host[i] * 4.0 * M_PI;
  if (pl->qbasis) {               // finalised before: the weighted operator works in the Y0 basis
    if (int rcb = build_all_bases(pl, nullptr)) return rcb;
    pl->qbasis = false;
  }
  DevBuf wd;
  int rc = upload(wd, w.data(), w.size() * 8);
  if (rc) return rc;
  rc = pl->yblk_w.ensure(pl->yblk.bytes);
  if (rc) {
    wd.release();
    return rc;
  }
  (void)hipMemset(pl->yblk_w.p, 0, pl->yblk_w.bytes);
  rc = build_basis(pl, wd.d(), nullptr, nullptr, pl->yblk_w.d());
  hipError_t e = hipDeviceSynchronize();
  wd.release();
  if (rc) return rc;
  if (e != hipSuccess) return fail(TEMX_EHIP, "basis kernel failed: %s", hipGetErrorString(e));
  std::vector<double> I((size_t)pl->K * pl->K, 0.0);
  for (int k = 0; k < pl->K; ++k) I[(size_t)k * pl->K + k] = 1.0;
  if (int rcg = set_ginv(pl, I.data())) return rcg;
  if (int rca = upload(pl->GinvA, I.data(), I.size() * 8)) return rca;
  // weighted rows of one latitude no longer share a basis row: every latitude-structured path is off
  // (the large-L class path too: its class basis ycls_l is unweighted)
  pl->sym = pl->cls = pl->lcls = false;
  pl->lone = pl->onepass = pl->op_valid = pl->xb_valid = false;
  pl->tem = false;                // splits / workspaces belong to the path: set_tem again
  pl->weighted = true;
  pl->finalized = true;
  pl->miss_built = pl->miss_valid = false;
  pl->bin_built = 0;
  return TEMX_OK;
} TEMX_CATCH

int temx_get_matrix(temx_plan* pl, int which, double* dst, void* stream) try {
  if (!pl || !dst) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  const size_t KK = (size_t)pl->K * pl->K * 8;
  switch (which) {
    case TEMX_MAT_Y0:
      HIPCHK(hipMemcpyAsync(dst, pl->Y0.p, (size_t)pl->N * pl->K * 8, hipMemcpyDeviceToDevice, st));
      return TEMX_OK;
    case TEMX_MAT_Y0P:
      HIPCHK(hipMemcpyAsync(dst, pl->Y0p.p, (size_t)pl->M * pl->K * 8, hipMemcpyDeviceToDevice, st));
      return TEMX_OK;
    case TEMX_MAT_GRAM:
      if (!pl->h_G_own.empty()) {       // finalised with the job's matrix: pl->G holds that one
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(dst, pl->h_G_own.data(), KK, hipMemcpyHostToDevice));
        return TEMX_OK;
      }
      HIPCHK(hipMemcpyAsync(dst, pl->G.p, KK, hipMemcpyDeviceToDevice, st));
      return TEMX_OK;
    case TEMX_MAT_GINV:
      if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
      HIPCHK(hipMemcpyAsync(dst, pl->GinvA.p, KK, hipMemcpyDeviceToDevice, st));
      return TEMX_OK;
    case TEMX_MAT_Y0INV:
      if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
      hipLaunchKernelGGL(y0inv_kernel, dim3((unsigned)((pl->N + 255) / 256)), dim3(256), 0, st, pl->Y0.d(),
                         pl->GinvA.d(), pl->N, pl->K, dst);
      HIPCHK(hipGetLastError());
      return TEMX_OK;
    case TEMX_MAT_GRAM2: {
      // this rank's share of Q^T Q (ncol-sharded callers all-reduce it and hand it to temx_plan_refine);
      // the identity when the plan does not run on a re-orthogonalised basis
      if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
      if (!pl->qbasis) {
        std::vector<double> I((size_t)pl->K * pl->K, 0.0);
        for (int k = 0; k < pl->K; ++k) I[(size_t)k * pl->K + k] = 1.0;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(dst, I.data(), KK, hipMemcpyHostToDevice));
        return TEMX_OK;
      }
      if (int rc2 = gram_of_q(pl)) return rc2;
      HIPCHK(hipMemcpyAsync(dst, pl->G2.p, KK, hipMemcpyDeviceToDevice, st));
      return TEMX_OK;
    }
    case TEMX_MAT_GX:
    case TEMX_MAT_GSUB: {
      if (!pl->os_built) return fail(TEMX_ESTATE, "the single-sweep tables are not built (temx_plan_set_tem on a plan that takes that form)");
      // this rank's own sums, whatever temx_plan_set_os_matrices has installed since: a second all-reduce of them
      // (a second temx_plan_set_tem, a second runner on the plan) gives the job's matrix again, not a multiple of it
      const std::vector<double>& h = which == TEMX_MAT_GX ? pl->h_Gx_own : pl->h_Gs;
      HIPCHK(hipStreamSynchronize(st));
      HIPCHK(hipMemcpy(dst, h.data(), h.size() * 8, hipMemcpyHostToDevice));
      return TEMX_OK;
    }
    case TEMX_MAT_COVERAGE:
      if (pl->miss_cov_D < 0) return fail(TEMX_ESTATE, "no masked run on this plan yet (TEMX_OPT_MISSING = 1)");
      HIPCHK(hipMemcpyAsync(dst, pl->mcov.p, (size_t)pl->M * pl->miss_cov_D * 8, hipMemcpyDeviceToDevice, st));
      return TEMX_OK;
    default:
      return fail(TEMX_EINVAL, "unknown matrix id %d", which);
  }
} TEMX_CATCH

// ncol-sharded single sweep: the two matrices of build_os_tables that sum over the rows -- Gx = Y0^T Y0ext [K][2L+1]
// and the Gram matrix of the reference subsample [KR][KR] -- summed over the ranks (all-reduce of
// temx_get_matrix(TEMX_MAT_GX / TEMX_MAT_GSUB)), handed back.
int temx_plan_set_os_matrices(temx_plan* pl, const double* Gx_host, const double* Gs_host) try {
  if (!pl || !Gx_host || !Gs_host) return fail(TEMX_EINVAL, "null argument");
  if (!pl->os_built) return fail(TEMX_ESTATE, "the single-sweep tables are not built");
  HIPCHK(hipSetDevice(pl->device));
  const int KR = pl->KR;
  std::vector<long double> Li;
  std::vector<double> Gi((size_t)KR * KR);
  if (spd_factor(Gs_host, KR, Li) != 0)
    return fail(TEMX_ERANK, "the subsample of latitude classes does not determine a degree-%d reference", KR - 1);
  inverse_from_factor(Li, KR, Gi.data());
  HIPCHK(hipDeviceSynchronize());
  if (int rc = upload(pl->Gsinv, Gi.data(), Gi.size() * 8)) return rc;
  if (int rc = upload(pl->Gx, Gx_host, (size_t)pl->K * pl->KX * 8)) return rc;
  pl->h_Gx.assign(Gx_host, Gx_host + (size_t)pl->K * pl->KX);
  if (int rc = os_upload_blocks(pl)) return rc;
  pl->os_need_global = false;
  pl->os_valid = false;
  return TEMX_OK;
} TEMX_CATCH

// ---- operator API --------------------------------------------------------------------------------
int temx_project(temx_plan* pl, const void* A, int dtype, int64_t D, double* B, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_project");
  if (!pl || !A || !B) return fail(TEMX_EINVAL, "null argument");
  if (D < 1 || D >= ((int64_t)1 << 28)) return fail(TEMX_EINVAL, "D must be in [1, 2^28)");
  HIPCHK(hipSetDevice(pl->device));
  if (bin_mode(pl)) return bin_project_op(pl, A, dtype, D, B, S_(stream));
  FieldPtrs<1> fp;
  fp.p[0] = A;
  if (pl->cls) {      // class sweep: one basis row per latitude class
    Split spc = choose_split(D, std::max<int64_t>(1, pl->cbatches / 4), CLS_PROJ_E_WPS * pl->num_cu, 4);
    int rcc = pl->partial.ensure((size_t)spc.nsplit * pl->K * D * 8);
    if (rcc) return rcc;
    if ((rcc = launch_project_cls<1>(pl, fp, dtype, D, nullptr, -1, pl->partial.d(), spc, S_(stream)))) return rcc;
    return launch_reduce(pl, pl->partial.d(), spc.nsplit, (int64_t)pl->K * D, B, S_(stream));
  }
  Split sp = choose_split(D, pl->nchunk, 2 * pl->num_cu);
  int rc = pl->partial.ensure((size_t)sp.nsplit * std::min(pl->K, 64) * D * 8);
  if (rc) return rc;
  return project_all<1>(pl, fp, dtype, D, nullptr, -1, sp, B, S_(stream));
} TEMX_CATCH

int temx_zonal_mean_from_sums(temx_plan* pl, const double* B, int64_t D, double* out, int native,
                              void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_zonal_mean_from_sums");
  if (pl && bin_refused(pl)) return bin_refuse("temx_zonal_mean_from_sums");
  if (!pl || !B || !out) return fail(TEMX_EINVAL, "null argument");
  if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
  HIPCHK(hipSetDevice(pl->device));
  int rc;
  if (!native) return launch_solve(pl, B, 1, D, nullptr, out, S_(stream));
  if ((rc = pl->opC.ensure((size_t)pl->K4 * D * 8))) return rc;
  if ((rc = launch_solve(pl, B, 1, D, pl->opC.d(), nullptr, S_(stream)))) return rc;
  return launch_recon(pl, D, pl->opC.d(), out, S_(stream));
} TEMX_CATCH

int temx_zonal_mean(temx_plan* pl, const void* A, int dtype, int64_t D, double* out, int native,
                    void* stream) try {
  if (!pl || !A || !out) return fail(TEMX_EINVAL, "null argument");
  if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
  if (miss_mode(pl)) return miss_zonal_mean(pl, A, dtype, D, out, native, S_(stream));
  if (bin_mode(pl)) return bin_zonal_mean(pl, A, dtype, D, out, native, S_(stream));
  int rc = pl->opB.ensure((size_t)pl->K * std::max<int64_t>(D, 1) * 8);
  if (rc) return rc;
  if ((rc = temx_project(pl, A, dtype, D, pl->opB.d(), stream))) return rc;
  return temx_zonal_mean_from_sums(pl, pl->opB.d(), D, out, native, stream);
} TEMX_CATCH

// ---- path selection: temx_plan_configure sets the options, the TEMX_* environment variables override them ------
// (the rules: tem_layout.hpp, form_choice)
static FormChoice form_choice(const temx_plan* pl) {
  return form_choice(pl->opt_form, bin_mode(pl), getenv("TEMX_TWO_PASS"), getenv("TEMX_ONE_PASS"), getenv("TEMX_SINGLE_SWEEP"));
}
// 1: loads of 4 rows x 16 columns (the MFMA tile), 0: loads of 1 row x 64 columns
static bool tile_map(int opt, const char* env) {
  if (const char* e = getenv(env)) return !strcmp(e, "tile");
  return opt == 1;
}
static bool os_barrier_wanted(const temx_plan* pl) {
  if (const char* e = getenv("TEMX_OS_SYNC")) return !strcmp(e, "barrier");
  return pl->opt_os_sync == 1;
}
static bool tracer_one_pass_wanted(const temx_plan* pl) {
  if (const char* e = getenv("TEMX_TRACER_ONE_PASS")) return e[0] == '1';
  return pl->opt_tracer_one_pass == 1;
}

static int bin_check(const temx_plan* pl);
static int bin_set_tem(temx_plan* pl);

int temx_plan_configure(temx_plan* pl, int option, int value) try {
  if (!pl) return fail(TEMX_EINVAL, "null plan");
  switch (option) {
    case TEMX_OPT_FORM:
      if (value < -1 || value > TEMX_FORM_NO_SINGLE_SWEEP) return fail(TEMX_EINVAL, "TEMX_OPT_FORM: unknown form %d", value);
      pl->opt_form = value;
      break;
    case TEMX_OPT_OS_MAP: pl->opt_os_map = value; break;
    case TEMX_OPT_OP_MAP: pl->opt_op_map = value; break;
    case TEMX_OPT_TRACER_ONE_PASS: pl->opt_tracer_one_pass = value; break;
    case TEMX_OPT_OS_SUBSAMPLE:
      if (value < 4) return fail(TEMX_EINVAL, "TEMX_OPT_OS_SUBSAMPLE: at least 4 class-groups");
      if (pl->os_built && value != pl->os_keep) return fail(TEMX_ESTATE, "the single-sweep tables of this plan are built: set the subsample before temx_plan_set_tem");
      pl->os_keep = value;
      break;
    case TEMX_OPT_SINGLE_SWEEP_MIN_GROUPS: pl->opt_single_sweep_min_groups = value; break;
    case TEMX_OPT_OS_CONTRACT: pl->opt_os_contract = value; break;
    case TEMX_OPT_MISSING:
      if (value != 0 && value != 1) return fail(TEMX_EINVAL, "TEMX_OPT_MISSING: 0 (raise) or 1 (mask), got %d", value);
      if (value == 1) {
        if (bin_mode(pl)) return fail(TEMX_EUNSUPPORTED, "missing-value mode is not available while latitude bins are in effect (TEMX_OPT_LAT_BINS)");
        if (int rc = miss_check(pl)) return rc;
      }
      pl->opt_missing = value;
      pl->miss_valid = false;
      break;
    case TEMX_OPT_MIN_COVERAGE:
      if (value < 0 || value > 1000) return fail(TEMX_EINVAL, "TEMX_OPT_MIN_COVERAGE: per mille in 0..1000, got %d", value);
      pl->opt_min_cov = value;
      break;
    case TEMX_OPT_MISSING_WEIGHT:
      if (value < 4 || value > 14) return fail(TEMX_EINVAL, "TEMX_OPT_MISSING_WEIGHT: tau = 10^-value, value in 4..14, got %d", value);
      pl->opt_miss_w = value;
      break;
    case TEMX_OPT_OS_SYNC:
      if (value != 0 && value != 1) return fail(TEMX_EINVAL, "TEMX_OPT_OS_SYNC: 0 (flags) or 1 (barriers), got %d", value);
      pl->opt_os_sync = value;
      break;
    case TEMX_OPT_LAT_BINS: {
      const int B = value == -1 ? BIN_DEFAULT : value;
      if (B != 0) {
        if (!bin_count_ok(B)) return fail(TEMX_EINVAL, "TEMX_OPT_LAT_BINS: 0 (off), -1 (default, %d) or one of 128, 256, 512, 1024, 2048, got %d", BIN_DEFAULT, value);
        if (int rc = bin_check(pl)) return rc;
        if (bin_degree(pl->L, B) == 0)
          return fail(TEMX_EINVAL, "TEMX_OPT_LAT_BINS: (L, B) = (%d, %d): no Chebyshev degree up to %d keeps the basis rows to %.0e; use more bins",
                      pl->L, B, BIN_MAX_DEGREE, BIN_BOUND);
      }
      pl->opt_lat_bins = B;
      pl->bin_J = B ? bin_degree(pl->L, B) : 0;
      break;
    }
    case TEMX_OPT_BIN_DEGREE: return fail(TEMX_EINVAL, "TEMX_OPT_BIN_DEGREE is chosen by the library (read it with temx_plan_option)");
    default: return fail(TEMX_EINVAL, "unknown option %d", option);
  }
  pl->tem = false;                // the choice is made in temx_plan_set_tem: call it (again)
  return TEMX_OK;
} TEMX_CATCH

int temx_plan_option(const temx_plan* pl, int option) try {
  if (!pl) return -1;
  switch (option) {
    case TEMX_OPT_FORM:
      if (miss_mode(pl)) return TEMX_FORM_MASKED;
      if (bin_mode(pl)) return TEMX_FORM_BINNED;
      return pl->os_on ? TEMX_FORM_SINGLE_SWEEP : ((pl->cls && pl->onepass) || (pl->lcls && pl->lone) ? TEMX_FORM_CLASS_SUMS : TEMX_FORM_TWO_PASS);
    case TEMX_OPT_OS_MAP: return tile_map(pl->opt_os_map, "TEMX_OS_MAP") ? 1 : 0;
    case TEMX_OPT_OP_MAP: return tile_map(pl->opt_op_map, "TEMX_OP_MAP") ? 1 : 0;
    case TEMX_OPT_TRACER_ONE_PASS: return tracer_one_pass_wanted(pl) ? 1 : 0;
    case TEMX_OPT_OS_SUBSAMPLE: return pl->os_keep;
    case TEMX_OPT_SINGLE_SWEEP_MIN_GROUPS: return pl->opt_single_sweep_min_groups;
    case TEMX_OPT_OS_CONTRACT: return pl->osc_lds ? 1 : 0;
    case TEMX_OPT_MISSING: return pl->opt_missing;
    case TEMX_OPT_MIN_COVERAGE: return pl->opt_min_cov;
    case TEMX_OPT_MISSING_WEIGHT: return pl->opt_miss_w;
    case TEMX_OPT_OS_SYNC: return os_barrier_wanted(pl) ? 1 : 0;
    case TEMX_OPT_LAT_BINS: return pl->opt_lat_bins;
    case TEMX_OPT_BIN_DEGREE: return pl->bin_J;
    default: return -1;
  }
} TEMX_CATCH

// ---- TEM pipeline --------------------------------------------------------------------------------
// temx_plan_set_tem, path by path: tem_layout.hpp decides, these allocate, fill and upload the work cuts (now, not at
// the first launch: launches must stay legal inside a stream capture).
static bool mem_free(size_t* fr) {
  size_t tot = 0;
  return hipMemGetInfo(fr, &tot) == hipSuccess;
}

// large-L class path: class sums first (kernels_cls.hpp) if both of their streams fit, the sliced two-pass sweeps if not
static int set_tem_large_cls(temx_plan* pl, const TemDims& d, const FormChoice& fc) {
  const LargeClsLayout l = tem_large_cls_layout(d, fc);
  size_t fr = 0;
  if (!(l.eligible && mem_free(&fr) && fits(l.csum, pl->csum.bytes, fr, l.pbuf) &&
        alloc_write_stream(pl->csum, l.csum) == TEMX_OK && pl->pbuf.ensure(l.pbuf) == TEMX_OK))
    return TEMX_OK;
  int rc;
  HIPCHK(hipMemset(pl->csum.p, 0, pl->csum.bytes));
  HIPCHK(hipMemset(pl->pbuf.p, 0, pl->pbuf.bytes));
  pl->sp_cproj4 = l.sp_cproj4;
  pl->sp_cflux = l.sp_cflux;
  pl->sp_lflux = l.sp_lflux;
  if ((rc = pl->partial.ensure(l.partial))) return rc;
  if ((rc = pl->Bs.ensure(l.Bs))) return rc;
  const int2* cuts_unused = nullptr;
  if ((rc = class_cuts_dev(pl, pl->sp_cproj4.nsplit, &cuts_unused, true))) return rc;
  pl->lone = true;
  return TEMX_OK;
}

// single sweep (no class-sum stream): its tables, then its buffers.  Too few distinct latitudes in the subsample
// (TEMX_ERANK) leave the plan on the class-sum form.
static int set_tem_single_sweep(temx_plan* pl, const TemDims& d) {
  int rc = build_os_tables(pl);
  if (rc == TEMX_ERANK) return TEMX_OK;
  if (rc) return rc;
  const SweepLayout s = tem_sweep_layout(d, pl->KX, pl->KR, pl->NQ, pl->sbatches);
  pl->sp_os = s.sp_os;
  pl->sp_os_s = s.sp_os_s;
  if ((rc = pl->partial.ensure(s.partial))) return rc;
  if ((rc = pl->Ax.ensure(s.Ax))) return rc;
  if ((rc = pl->Axs.ensure(s.Axs))) return rc;
  if ((rc = pl->osAt.ensure(s.osAt))) return rc;
  if ((rc = pl->osAb.ensure(s.osAb))) return rc;
  if ((rc = pl->rho.ensure(s.rho))) return rc;
  if ((rc = pl->rho0.ensure(s.rho0))) return rc;
  HIPCHK(hipMemset(pl->rho0.p, 0, pl->rho0.bytes));
  const int2* cu = nullptr;
  if ((rc = os_cuts_dev(pl, false, pl->sp_os.nsplit, &cu))) return rc;
  if ((rc = os_cuts_dev(pl, true, pl->sp_os_s.nsplit, &cu))) return rc;
  pl->os_on = true;
  return TEMX_OK;
}

// class path: the two-pass cuts; the one-pass form where it is wanted and the class sums find room (no memory: the
// two-pass form stays); the single sweep where that is wanted on top
static int set_tem_cls(temx_plan* pl, const TemDims& d, const FormChoice& fc) {
  int rc;
  const ClsLayout c = tem_cls_layout(d, fc);
  pl->sp_cproj4 = c.sp_cproj4;
  pl->sp_cproj1 = c.sp_cproj1;
  pl->sp_ceddy = c.sp_ceddy;
  if ((rc = pl->partial.ensure(c.partial))) return rc;
  bool have = c.want_onepass && pl->csum.bytes >= c.csum;
  size_t fr = 0;
  if (c.want_onepass && !have && mem_free(&fr) && fits(c.csum, pl->csum.bytes, fr) &&
      alloc_write_stream(pl->csum, c.csum) == TEMX_OK) {
    // lanes beyond a ragged last d-tile are never written but are read (and ignored) by the flux kernel
    HIPCHK(hipMemset(pl->csum.p, 0, pl->csum.bytes));
    have = true;
  }
  if (have) {
    const OnePassLayout o = tem_onepass_layout(d, fc, os_supported(pl), pl->opt_single_sweep_min_groups);
    pl->onepass = true;
    pl->sp_cproj4 = o.sp_cproj4;
    pl->sp_cflux = o.sp_cflux;
    pl->sp_copw = o.sp_copw;
    if ((rc = pl->partial.ensure(o.partial))) return rc;
    if ((rc = pl->Pq.ensure(o.Pq))) return rc;
    if (o.want_os && (rc = set_tem_single_sweep(pl, d))) return rc;
  }
  const int2* cuts_unused = nullptr;
  if (pl->onepass && (rc = class_cuts_dev(pl, pl->sp_cproj4.nsplit, &cuts_unused, true))) return rc;
  if (pl->onepass && (rc = class_cuts_dev(pl, pl->sp_copw.nsplit * 4, &cuts_unused, true))) return rc;
  for (int nsub : {pl->sp_cproj4.nsplit, pl->sp_cproj1.nsplit, pl->sp_ceddy.nsplit * (8 / d.edpw())})
    if ((rc = class_cuts_dev(pl, nsub, &cuts_unused))) return rc;
  return TEMX_OK;
}

// mirror-paired path
static int set_tem_sym(temx_plan* pl, const TemDims& d) {
  const SymLayout s = tem_sym_layout(d);
  pl->sp_sproj4 = s.sp_sproj4;
  pl->sp_sproj1 = s.sp_sproj1;
  pl->sp_seddy = s.sp_seddy;
  return pl->partial.ensure(s.partial);
}

int temx_plan_set_tem(temx_plan* pl, int nlev, int64_t nt, const double* p_pa_host, double p0) try {
  if (!pl || !p_pa_host) return fail(TEMX_EINVAL, "null argument");
  if (nlev < 2 || nt < 1) return fail(TEMX_EINVAL, "need nlev >= 2 and nt >= 1");
  if ((int64_t)nlev * nt >= ((int64_t)1 << 28)) return fail(TEMX_EINVAL, "nlev*nt must be < 2^28");
  if (pl->M < 2) return fail(TEMX_EINVAL, "need at least 2 zonal-mean latitudes");
  HIPCHK(hipSetDevice(pl->device));
  std::vector<double> p(p_pa_host, p_pa_host + nlev);
  for (int j = 1; j < nlev; ++j)
    if (!(p[j] > p[j - 1])) return fail(TEMX_EINVAL, "pressure must be strictly ascending (front end flips)");
  // a failure below must not leave an earlier configuration half replaced: the plan is unconfigured
  // (tem_ready fails) until the last allocation has succeeded
  pl->tem = false;
  pl->onepass = pl->lone = pl->op_valid = pl->xb_valid = pl->tq_valid = false;
  pl->os_on = pl->os_valid = false;
  pl->miss_valid = pl->mt_valid = false;   // the masked coefficients describe the columns of the previous configuration
  pl->os_tile = tile_map(pl->opt_os_map, "TEMX_OS_MAP");
  {
    const char* e = getenv("TEMX_OS_CONTRACT");
    pl->osc_lds = e ? !strcmp(e, "lds") : pl->opt_os_contract == 1;
  }
  pl->op_tile = tile_map(pl->opt_op_map, "TEMX_OP_MAP");
  pl->os_barrier = os_barrier_wanted(pl);
  pl->nlev = nlev;
  pl->nt = nt;
  pl->D = (int64_t)nlev * nt;
  pl->tD = pl->D;
  pl->tnt = nt;
  pl->tt0 = 0;
  pl->p0 = p0;
  int rc;
  const TemTables tt = tem_tables(p, nt, p0, pl->lat_out_deg);
  if ((rc = upload(pl->p, p))) return rc;
  if ((rc = upload(pl->pg, tt.pg))) return rc;
  if ((rc = upload(pl->lg, tt.lg))) return rc;
  if ((rc = upload(pl->coslat, tt.coslat))) return rc;
  if ((rc = upload(pl->fcor, tt.fcor))) return rc;
  if ((rc = upload(pl->colscale, tt.colscale))) return rc;

  // what runs, how it is cut and what it needs: tem_layout.hpp.  `partial` grows stage by stage, as far as the stages
  // that apply ask for; the class-sum stream csum is placed after the first of them.
  const TemDims d = tem_dims(pl);
  const FormChoice fc = form_choice(pl);
  const BaseLayout b = tem_base_layout(d);
  pl->sp_proj4 = b.sp_proj4;
  pl->sp_eddy = b.sp_eddy;
  pl->sp_proj1 = b.sp_proj1;
  if ((rc = pl->partial.ensure(b.partial))) return rc;
  if ((rc = pl->B4.ensure(b.B4))) return rc;
  if ((rc = pl->B3.ensure(b.B3))) return rc;
  if ((rc = pl->C4.ensure(b.C4))) return rc;
  if ((rc = pl->zb.ensure(b.zb))) return rc;
  if ((rc = pl->partial.ensure(b.partial_unfused))) return rc;
  if (pl->lcls && (rc = set_tem_large_cls(pl, d, fc))) return rc;
  if (pl->cls && (rc = set_tem_cls(pl, d, fc))) return rc;
  if (pl->sym && (rc = set_tem_sym(pl, d))) return rc;
  if (bin_mode(pl) && (rc = bin_set_tem(pl))) return rc;   // tables (first time) and the workspace of the binned sweeps
  pl->tem = true;
  return TEMX_OK;
} TEMX_CATCH

static int tem_ready(temx_plan* pl) {
  if (!pl) return fail(TEMX_EINVAL, "null plan");
  if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
  if (!pl->tem) return fail(TEMX_ESTATE, "temx_plan_set_tem has not been called");
  return TEMX_OK;
}

int temx_tem_stage1(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap,
                    int dtype, double* B4, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_stage1");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_stage1");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!ua || !va || !ta || !wap || !B4) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  FieldPtrs<4> fp;
  fp.p[0] = ua; fp.p[1] = va; fp.p[2] = ta; fp.p[3] = wap;
  if (pl->large) set_tail(pl, 0, pl->nt);
  if (pl->large && pl->lone) {   // class sums first, then their projection slice by slice
    pl->op_valid = false;
    if ((rc = launch_class_sums(pl, fp, dtype, st))) return rc;
    if ((rc = project_sums<4>(pl, pl->csum.d(), 7, 0, B4, st))) return rc;
    pl->op_valid = true;
    return TEMX_OK;
  }
  if (pl->large) return project_all<4>(pl, fp, dtype, pl->D, pl->colscale.d(), 2, pl->sp_proj4, B4, st);
  TimedLaunch tl{};
  time_begin(pl, 0, st, tl);
  const bool sp4 = sym_project(pl, 4);
  const Split& sp = pl->cls ? pl->sp_cproj4 : (sp4 ? pl->sp_sproj4 : pl->sp_proj4);
  const bool op = pl->cls && pl->onepass;
  set_tail(pl, 0, pl->nt);
  pl->op_valid = false;
  pl->os_valid = false;
  pl->c4_valid = false;          // C4 still describes the previous fields until a stage-2 solve has run
  pl->tq_valid = false;          // tracer class sums pair with the v, omega sums of one TEM run
  rc = op      ? launch_sweep_op<0>(pl, fp, dtype, pl->partial.d(), sp, st)
       : pl->cls ? launch_project_cls<4>(pl, fp, dtype, pl->D, pl->colscale.d(), 2, pl->partial.d(), sp, st)
       : sp4   ? launch_project_sym<4>(pl, fp, dtype, pl->D, pl->colscale.d(), 2, pl->partial.d(), sp, st)
               : launch_project<4>(pl, fp, dtype, pl->D, pl->colscale.d(), 2, pl->partial.d(), sp, st);
  time_end(pl, 0, st, tl);
  if (rc) return rc;
  const int64_t KD = (int64_t)pl->K * pl->D;
  if (!op) return launch_reduce(pl, pl->partial.d(), sp.nsplit, 4 * KD, B4, st);
  // one-pass form: 7 slabs per split -- the four fields, then the products u v, u omega, v theta
  if ((rc = launch_reduce(pl, pl->partial.d(), sp.nsplit, 4 * KD, B4, st, 7 * KD))) return rc;
  if ((rc = launch_reduce(pl, pl->partial.d() + 4 * KD, sp.nsplit, 3 * KD, pl->Pq.d(), st, 7 * KD))) return rc;
  pl->op_valid = true;           // csum / Pq now describe these fields (temx_tem_stage2_from_sums)
  return TEMX_OK;
} TEMX_CATCH

// ---- large-L (K > 64) second sweep: the fused eddy kernel keeps all coefficients of a d-tile in LDS,
// which stops at 64 harmonics.  Here the native zonal means are materialised by accumulating
// reconstruction passes (64 harmonics each), the eddies/products by one elementwise kernel, and
// the products are projected slice by slice.  ~8x the HBM traffic of the fused path; correct for
// any L <= 511.
static int large_ws(temx_plan* pl) {
  const size_t nd = (size_t)pl->N * pl->D * 8;
  int rc;
  // 8 arrays of ncol x nlev x nt doubles (107 GB at ne120 x 72 x 30): say so before the allocator does
  size_t fr = 0, tot = 0;
  const size_t have = pl->XB.bytes + pl->P3.bytes;
  if (have < 8 * nd && hipMemGetInfo(&fr, &tot) == hipSuccess && 8 * nd - have > fr)
    return fail(TEMX_ENOMEM, "the unfused second sweep (L > 63 without latitude classes, or a weighted plan) needs "
                             "%zu bytes of workspace (8 x ncol x nlev x nt doubles), %zu are free; process the "
                             "snapshots in smaller blocks (temx_plan_set_tem with a smaller nt)", 8 * nd - have, fr);
  if ((rc = pl->XB.ensure(5 * nd))) return rc;     // ub vb thetab wapb (+ qb for tracers), native
  return pl->P3.ensure(3 * nd);
}

static int launch_eddy_from_xbar(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, const FieldPtrs<4>& xb,
                                 const double* colscale, const EddyOut& eo, hipStream_t st, int64_t nrows = -1) {
  if (nrows < 0) nrows = pl->N;
  dim3 grid((unsigned)(pl->num_cu * 8)), block(256);
  if (dtype == TEMX_F64)
    hipLaunchKernelGGL(eddy_from_xbar_kernel<double>, grid, block, 0, st, fp, xb, nrows, pl->D, colscale, eo);
  else if (dtype == TEMX_F32)
    hipLaunchKernelGGL(eddy_from_xbar_kernel<float>, grid, block, 0, st, fp, xb, nrows, pl->D, colscale, eo);
  else
    return bad_dtype();
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

static FieldPtrs<4> native_means(temx_plan* pl, int a, int b, int c, int d) {
  const int64_t nd = pl->N * pl->D;
  FieldPtrs<4> xb;
  xb.p[0] = pl->XB.d() + a * nd; xb.p[1] = pl->XB.d() + b * nd;
  xb.p[2] = pl->XB.d() + c * nd; xb.p[3] = pl->XB.d() + d * nd;
  return xb;
}

// native zonal means of the four fields from the coefficients of the last solve (large-L paths)
static int ensure_xb(temx_plan* pl, hipStream_t st) {
  if (pl->xb_valid) return TEMX_OK;
  int rc;
  if ((rc = large_ws(pl))) return rc;
  const int64_t nd = pl->N * pl->D;
  for (int f = 0; f < 4; ++f)
    if ((rc = launch_recon(pl, pl->D, pl->C4.d() + (int64_t)f * pl->K4 * pl->D, pl->XB.d() + f * nd, st))) return rc;
  pl->xb_valid = true;
  return TEMX_OK;
}

static int tem_stage2_large(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, const double* B4, double* B3,
                            hipStream_t st) {
  int rc;
  if ((rc = large_ws(pl))) return rc;
  const int64_t nd = pl->N * pl->D;
  if ((rc = launch_solve(pl, B4, 4, pl->D, pl->C4.d(), pl->zb.d(), st))) return rc;
  pl->c4_valid = true;
  for (int f = 0; f < 4; ++f)
    if ((rc = launch_recon(pl, pl->D, pl->C4.d() + (int64_t)f * pl->K4 * pl->D, pl->XB.d() + f * nd, st))) return rc;
  EddyOut eo{};
  FieldPtrs<3> f3;
  for (int i = 0; i < 3; ++i) {
    eo.p[4 + i] = pl->P3.d() + i * nd;
    f3.p[i] = eo.p[4 + i];
  }
  pl->xb_valid = true;
  if ((rc = launch_eddy_from_xbar(pl, fp, dtype, native_means(pl, 0, 1, 2, 3), pl->colscale.d(), eo, st))) return rc;
  return project_all<3>(pl, f3, TEMX_F64, pl->D, nullptr, -1, pl->sp_proj1, B3, st);
}

int temx_tem_stage2(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap,
                    int dtype, const double* B4, double* B3, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_stage2");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_stage2");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!ua || !va || !ta || !wap || !B4 || !B3) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  set_tail(pl, 0, pl->nt);
  if (unfused_stage2(pl)) return tem_stage2_large(pl, four(ua, va, ta, wap), dtype, B4, B3, st);
  // C = G^-1 B4 and the four zonal means ub vb thetab wapb -> zb[0..3]
  if ((rc = launch_solve(pl, B4, 4, pl->D, pl->C4.d(), pl->zb.d(), st))) return rc;
  pl->c4_valid = true;
  TimedLaunch tl{};
  time_begin(pl, 1, st, tl);
  rc = run_eddy<0>(pl, four(ua, va, ta, wap), dtype, pl->C4.d(), pl->partial.d(), nullptr, st);
  time_end(pl, 1, st, tl);
  if (rc) return rc;
  return launch_reduce(pl, pl->partial.d(), eddy_slabs(pl), (int64_t)3 * pl->K * pl->D, B3, st);
} TEMX_CATCH

int temx_tem_stage2_from_sums(temx_plan* pl, const double* B4, double* B3, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_stage2_from_sums");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_stage2_from_sums");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!B4 || !B3) return fail(TEMX_EINVAL, "null argument");
  if (!((pl->cls && pl->onepass) || (pl->large && pl->lone)))
    return fail(TEMX_ESTATE, "the plan does not run the one-pass class path (temx_plan_one_pass)");
  if (!pl->op_valid)
    return fail(TEMX_ESTATE, "no class sums: temx_tem_stage1 must precede temx_tem_stage2_from_sums");
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  if (!tail_is_whole(pl)) return fail(TEMX_ESTATE, "a time-sliced tail ran since the last temx_tem_stage1");
  if ((rc = launch_solve(pl, B4, 4, pl->D, pl->C4.d(), pl->zb.d(), st))) return rc;
  pl->c4_valid = true;
  if (pl->large) {
    if ((rc = launch_flux_large(pl, pl->C4.d(), st))) return rc;
    pl->xb_valid = false;          // the native means are not materialised on this path
    return project_sums<3>(pl, pl->pbuf.d(), 3, 0, B3, st);
  }
  TimedLaunch tl{};
  time_begin(pl, 1, st, tl);
  rc = launch_flux_cls<0>(pl, pl->C4.d(), pl->partial.d(), pl->sp_cflux, st);
  time_end(pl, 1, st, tl);
  if (rc) return rc;
  // B3 = (projections of u v, u omega, v theta from sweep 1) + (projected corrections)
  return launch_reduce(pl, pl->partial.d(), pl->sp_cflux.nsplit, (int64_t)3 * pl->K * pl->D, B3, st, -1,
                       pl->Pq.d());
} TEMX_CATCH

int temx_tem_stage3(temx_plan* pl, const double* B3, double* results, double* zonal, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_stage3");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_stage3");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!B3 || !results) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  if (!tail_is_whole(pl))
    return fail(TEMX_ESTATE, "the zonal means in the plan are those of a time slice (temx_tem_os_tail); stage 3 needs a "
                             "temx_tem_stage2 / stage2_from_sums on the whole run first");
  return tem_stage3_impl(pl, B3, results, zonal, S_(stream));
} TEMX_CATCH

// flux zonal means, derivatives, psi, integral and the ten diagnostics for the snapshots of the tail (pl->tnt of them;
// zb[0..3] hold the zonal means of the four fields for the same snapshots)
static int tem_stage3_impl(temx_plan* pl, const double* B3, double* results, double* zonal, hipStream_t st) {
  int rc;
  const int64_t Dt = pl->tD;
  const int64_t MD = (int64_t)pl->M * Dt;
  // flux zonal means upvpb upwappb vptpb -> zb[4..6]
  if ((rc = launch_solve(pl, B3, 3, Dt, nullptr, pl->zb.d() + 4 * MD, st))) return rc;
  return tem_epilogue(pl, results, zonal, st);
}

// int_vbdp, derivatives, psi and the ten diagnostics from the seven zonal means in zb[0..6], [8][M][nlev][nts]: the
// plan's own buffer (tem_epilogue) or the caller's (temxc_tem_from_zonal_means); reads the plan's tables only
static int tem_epilogue_on(temx_plan* pl, double* zb, int64_t nts, double* results, double* zonal, hipStream_t st) {
  const int64_t Dt = (int64_t)pl->nlev * nts;
  const int64_t MD = (int64_t)pl->M * Dt;
  // int_vbdp -> zb[7]: by a wavefront scan; inside the epilogue only for short columns on small zonal grids
  // (measured: at nlev = 72 the O(nlev) loop per point costs what the extra launch saves, at 128 more)
  EpiTables tb{pl->p.d(), pl->pg.d(), pl->lg.d(), pl->coslat.d(), pl->fcor.d()};
  static const bool epi_wg = !(getenv("TEMX_EPI_WG") && atoi(getenv("TEMX_EPI_WG")) == 0);   // A/B only
  if (epi_wg && Dt <= EPI_WG_MAXD) {          // small zonal grid: the scan inside the epilogue, one workgroup per latitude
    hipLaunchKernelGGL(tem_epilogue_kernel<2>, dim3((unsigned)pl->M), dim3(256), 0, st, zb, pl->M, pl->nlev, nts, tb,
                       pl->p0, results, zonal);
  } else if (pl->nlev > 40 || MD > ((int64_t)1 << 17)) {
    const int64_t ncols = (int64_t)pl->M * nts;
    hipLaunchKernelGGL(pint_scan_kernel, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, st, zb + 1 * MD,
                       pl->p.d(), pl->M, pl->nlev, nts, zb + 7 * MD);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(tem_epilogue_kernel<0>, dim3((unsigned)((MD + 255) / 256)), dim3(256), 0, st, zb,
                       pl->M, pl->nlev, nts, tb, pl->p0, results, zonal);
  } else {
    hipLaunchKernelGGL(tem_epilogue_kernel<1>, dim3((unsigned)((MD + 255) / 256)), dim3(256), 0, st, zb,
                       pl->M, pl->nlev, nts, tb, pl->p0, results, zonal);
  }
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

static int tem_epilogue(temx_plan* pl, double* results, double* zonal, hipStream_t st) {
  return tem_epilogue_on(pl, pl->zb.d(), pl->tnt, results, zonal, st);
}

// ---- the single sweep in three steps (ncol-sharded jobs exchange between them; see include/temx.h) -----------
static int os_ready(temx_plan* pl) {
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!pl->os_on) return fail(TEMX_ESTATE, "the plan does not run the single-sweep form (temx_plan_single_sweep)");
  if (pl->os_need_global)
    return fail(TEMX_ESTATE, "ncol-sharded single sweep: temx_plan_set_os_matrices with the all-reduced TEMX_MAT_GX / TEMX_MAT_GSUB first");
  return TEMX_OK;
}
static int slices_ok(const temx_plan* pl, int nslices) {
  if (nslices < 1 || nslices > pl->nt)
    return fail(TEMX_EINVAL, "nslices = %d: a time-sliced tail needs 1 <= nslices <= nt = %lld", nslices, (long long)pl->nt);
  return TEMX_OK;
}

int temx_tem_os_prepass(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap, int dtype,
                        double* As, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_os_prepass");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_os_prepass");
  int rc = os_ready(pl);
  if (rc) return rc;
  if (!ua || !va || !ta || !wap || !As) return fail(TEMX_EINVAL, "null argument");
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  HIPCHK(hipSetDevice(pl->device));
  return os_prepass(pl, four(ua, va, ta, wap), dtype, As, S_(stream));
} TEMX_CATCH

int temx_tem_os_sweep(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap, int dtype,
                      const double* As, int nslices, double* proj, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_os_sweep");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_os_sweep");
  int rc = os_ready(pl);
  if (rc) return rc;
  if (!ua || !va || !ta || !wap || !As || !proj) return fail(TEMX_EINVAL, "null argument");
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  if ((rc = slices_ok(pl, nslices))) return rc;
  HIPCHK(hipSetDevice(pl->device));
  return os_sweep(pl, four(ua, va, ta, wap), dtype, As, nslices, proj, S_(stream));
} TEMX_CATCH

int temx_tem_os_tail(temx_plan* pl, const double* proj_slice, int64_t t0, int64_t nts, double* results, double* zonal,
                     void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_os_tail");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_os_tail");
  int rc = os_ready(pl);
  if (rc) return rc;
  if (!proj_slice || !results) return fail(TEMX_EINVAL, "null argument");
  if (t0 < 0 || nts < 1 || t0 + nts > pl->nt)
    return fail(TEMX_EINVAL, "snapshots [%lld, %lld) are not inside the run (nt = %lld)", (long long)t0, (long long)(t0 + nts), (long long)pl->nt);
  HIPCHK(hipSetDevice(pl->device));
  return os_tail(pl, proj_slice, t0, nts, results, zonal, S_(stream));
} TEMX_CATCH

static int tracers_args(const temx_plan* pl, int nq, const void* const* q_host, const void* va, const void* wap, int dtype) {
  if (nq != 1 && nq != 2) return fail(TEMX_EINVAL, "nq = %d: one or two tracers per sweep", nq);
  if (!q_host || !q_host[0] || (nq == 2 && !q_host[1]) || !va || !wap) return fail(TEMX_EINVAL, "null argument");
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  if (nq == 2 && (pl->os_tile || pl->osc_lds))
    return fail(TEMX_EUNSUPPORTED, "two tracers per sweep: not with TEMX_OPT_OS_MAP = tile / TEMX_OPT_OS_CONTRACT = lds");
  return TEMX_OK;
}

int temx_tracers_os_prepass(temx_plan* pl, int nq, const void* const* q_host, const void* va, const void* wap, int dtype,
                            double* Asq, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracers_os_prepass");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tracers_os_prepass");
  int rc = os_ready(pl);
  if (rc) return rc;
  if ((rc = tracers_args(pl, nq, q_host, va, wap, dtype))) return rc;
  if (!Asq) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  return tracer_os_prepass(pl, nq, tracer_fields(nq, q_host, va, wap), dtype, Asq, S_(stream));
} TEMX_CATCH

int temx_tracers_os_sweep(temx_plan* pl, int nq, const void* const* q_host, const void* va, const void* wap, int dtype,
                          const double* Asq, int nslices, double* projq, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracers_os_sweep");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tracers_os_sweep");
  int rc = os_ready(pl);
  if (rc) return rc;
  if ((rc = tracers_args(pl, nq, q_host, va, wap, dtype))) return rc;
  if (!Asq || !projq) return fail(TEMX_EINVAL, "null argument");
  if ((rc = slices_ok(pl, nslices))) return rc;
  HIPCHK(hipSetDevice(pl->device));
  return tracer_os_sweep(pl, nq, tracer_fields(nq, q_host, va, wap), dtype, Asq, nslices, projq, S_(stream));
} TEMX_CATCH

int temx_tracers_os_tail(temx_plan* pl, int nq, const double* projq_slice, double* const* tres_host, double* const* tzon_host,
                         void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracers_os_tail");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tracers_os_tail");
  int rc = os_ready(pl);
  if (rc) return rc;
  if (nq != 1 && nq != 2) return fail(TEMX_EINVAL, "nq = %d: one or two tracers per sweep", nq);
  if (!projq_slice || !tres_host || !tres_host[0] || (nq == 2 && !tres_host[1])) return fail(TEMX_EINVAL, "null argument");
  if (!pl->os_valid || !pl->c4_valid)
    return fail(TEMX_ESTATE, "the tracers' tail needs the state of a temx_tem_os_tail on the same snapshots");
  HIPCHK(hipSetDevice(pl->device));
  if ((rc = tracer_os_ws(pl, nq))) return rc;
  return tracer_os_tail(pl, nq, projq_slice, tres_host, tzon_host, S_(stream));
} TEMX_CATCH

// stages 2b + 3 on a time slice, from raw sums of any form of the sweeps: B4s [4][K][nlev][nts], B3s [3][K][nlev][nts]
int temx_tem_tail_from_sums(temx_plan* pl, const double* B4s, const double* B3s, int64_t t0, int64_t nts, double* results,
                            double* zonal, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_tail_from_sums");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_tail_from_sums");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!B4s || !B3s || !results) return fail(TEMX_EINVAL, "null argument");
  if (t0 < 0 || nts < 1 || t0 + nts > pl->nt)
    return fail(TEMX_EINVAL, "snapshots [%lld, %lld) are not inside the run (nt = %lld)", (long long)t0, (long long)(t0 + nts), (long long)pl->nt);
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  set_tail(pl, t0, nts);
  pl->c4_valid = pl->os_valid = false;                        // zb describes the slice from here on
  if ((rc = launch_solve(pl, B4s, 4, pl->tD, nullptr, pl->zb.d(), st))) return rc;
  return tem_stage3_impl(pl, B3s, results, zonal, st);
} TEMX_CATCH

// Cut rows of [nlev][nt] columns into the time slices a reduce-scatter wants: out[w][row][lev][t - t0(w)], slice w
// padded to rows * nlev * ceil(nt / nslices) doubles (kernels.hpp, SliceMap).
int temx_time_slices(temx_plan* pl, const double* B, int64_t rows, int nslices, double* out, void* stream) try {
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!B || !out || rows < 1) return fail(TEMX_EINVAL, "bad argument");
  if ((rc = slices_ok(pl, nslices))) return rc;
  HIPCHK(hipSetDevice(pl->device));
  return launch_reduce(pl, B, 1, rows * pl->D, out, S_(stream), -1, nullptr, slice_map(pl, nslices, rows, 0));
} TEMX_CATCH

// ---- missing-value mode (kernels_miss.hpp): tables, the masked TEM run and the masked operator ------------------
// configurations the masked path serves (checked at temx_plan_configure and again before every masked run)
static int miss_check(const temx_plan* pl) {
  if (pl->K > 64) return fail(TEMX_EUNSUPPORTED, "missing-value mode: L = %d, this version supports L <= 63", pl->L);
  if (pl->weighted) return fail(TEMX_EUNSUPPORTED, "missing-value mode is not available on a weights-mode plan");
  if (pl->finalized && pl->rank < pl->K)
    return fail(TEMX_EUNSUPPORTED, "missing-value mode: the plan was finalised through the pseudo-inverse (rank %d < K = %d; "
                                   "fewer distinct latitudes than harmonics)", pl->rank, pl->K);
  return TEMX_OK;
}

// Built once per basis: the raw rows of the e projection and the tables of the per-d systems (kernels_miss.hpp)
static int miss_setup(temx_plan* pl) {
  if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
  if (int rc = miss_check(pl)) return rc;
  if (pl->miss_built) return TEMX_OK;
  const int K = pl->K, NE = 2 * pl->L + 1, NQ = 2 * pl->L + 1, TBE = 2 * pl->TB;
  int rc;
  pl->NE = NE;
  pl->NQM = NQ;
  const int64_t npad = pl->nchunk * 16;
  if ((rc = pl->eblk.ensure((size_t)pl->nchunk * 4 * TBE * 16 * 8))) return rc;
  hipLaunchKernelGGL(miss_basis_kernel, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, 0, pl->x.d(), pl->N, npad, NE,
                     TBE, pl->eblk.d());
  HIPCHK(hipGetLastError());
  // Q^T Q over this plan's rows (Y0^T Y0 when the plan keeps the Y0 basis)
  std::vector<double> G2((size_t)K * K), T((size_t)K * K, 0.0);
  if (pl->qbasis) {
    if ((rc = gram_of_q(pl))) return rc;
    HIPCHK(hipMemcpy(G2.data(), pl->G2.p, G2.size() * 8, hipMemcpyDeviceToHost));
    T = pl->h_T;
  } else {
    HIPCHK(hipMemcpy(G2.data(), pl->G.p, G2.size() * 8, hipMemcpyDeviceToHost));
    for (int l = 0; l < K; ++l) T[(size_t)l * K + l] = 1.0;
  }
  std::vector<double> xs((size_t)pl->N);
  HIPCHK(hipMemcpy(xs.data(), pl->x.p, xs.size() * 8, hipMemcpyDeviceToHost));
  // pl->h_Ginv: the default operator, coefficients = Gi Q^T a
  if ((rc = upload(pl->mtab, miss_tables(G2.data(), T.data(), pl->h_Ginv.data(), xs.data(), pl->N, K, pl->L)))) return rc;
  HIPCHK(hipDeviceSynchronize());
  pl->miss_built = true;
  return TEMX_OK;
}

// temx_tem_run in missing-value mode: two reads of the four fields, per-d masked systems, the shared epilogue
static int miss_tem_run(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, double* results, double* zonal, hipStream_t st) {
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  int rc;
  if ((rc = miss_setup(pl))) return rc;
  const int64_t D = pl->D, KD = (int64_t)pl->K * D, MD = (int64_t)pl->M * D;
  if ((rc = pl->mB.ensure((size_t)(4 * KD + (int64_t)pl->NE * D) * 8))) return rc;
  if ((rc = pl->mC.ensure((size_t)4 * pl->K4 * D * 8))) return rc;
  if ((rc = pl->mCcov.ensure((size_t)pl->K4 * D * 8))) return rc;
  if ((rc = pl->mcov.ensure((size_t)MD * 8))) return rc;
  set_tail(pl, 0, pl->nt);
  pl->miss_valid = pl->mt_valid = false;
  pl->op_valid = pl->os_valid = pl->c4_valid = pl->tq_valid = pl->xb_valid = false;
  pl->miss_cov_D = -1;
  const double* E = pl->mB.d() + 4 * KD;
  TimedLaunch tl{};
  time_begin(pl, 0, st, tl);
  rc = launch_miss_project<4>(pl, fp, dtype, D, pl->colscale.d(), 2, pl->mB.d(), st);
  time_end(pl, 0, st, tl);
  if (rc) return rc;
  // coefficients of u v theta omega, ub vb thetab wapb -> zb[0..3], coverage
  if ((rc = launch_miss_system<4>(pl, pl->mB.d(), E, D, pl->mC.d(), pl->mCcov.d(), pl->zb.d(), pl->mcov.d(), st))) return rc;
  TimedLaunch tl2{};
  time_begin(pl, 1, st, tl2);
  rc = launch_miss_eddy(pl, fp, dtype, st);
  time_end(pl, 1, st, tl2);
  if (rc) return rc;
  const int slabs = pl->sp_eddy.nsplit * (8 / pl->sp_eddy.dpw);
  if ((rc = launch_reduce(pl, pl->partial.d(), slabs, 3 * KD, pl->B3.d(), st))) return rc;
  // upvpb upwappb vptpb -> zb[4..6] with the same systems
  if ((rc = launch_miss_system<3>(pl, pl->B3.d(), E, D, nullptr, nullptr, pl->zb.d() + 4 * MD, nullptr, st))) return rc;
  if ((rc = tem_epilogue(pl, results, zonal, st))) return rc;
  pl->miss_valid = true;
  pl->miss_cov_D = D;
  return TEMX_OK;
}

// temx_zonal_mean in missing-value mode (the field's own finiteness is the mask)
static int miss_zonal_mean(temx_plan* pl, const void* A, int dtype, int64_t D, double* out, int native, hipStream_t st) {
  if (D < 1 || D >= ((int64_t)1 << 28)) return fail(TEMX_EINVAL, "D must be in [1, 2^28)");
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  HIPCHK(hipSetDevice(pl->device));
  int rc;
  if ((rc = miss_setup(pl))) return rc;
  const int64_t KD = (int64_t)pl->K * D, MD = (int64_t)pl->M * D;
  if ((rc = pl->opB.ensure((size_t)(KD + (int64_t)pl->NE * D) * 8))) return rc;
  if ((rc = pl->mcov.ensure((size_t)MD * 8))) return rc;
  pl->miss_cov_D = -1;
  FieldPtrs<1> fp;
  fp.p[0] = A;
  if ((rc = launch_miss_project<1>(pl, fp, dtype, D, nullptr, -1, pl->opB.d(), st))) return rc;
  const double* E = pl->opB.d() + KD;
  if (!native) {
    if ((rc = launch_miss_system<1>(pl, pl->opB.d(), E, D, nullptr, nullptr, out, pl->mcov.d(), st))) return rc;
  } else {
    if ((rc = pl->opC.ensure((size_t)2 * pl->K4 * D * 8))) return rc;
    if ((rc = pl->mZ.ensure((size_t)MD * 8))) return rc;
    double* C = pl->opC.d();
    double* Ccov = C + (int64_t)pl->K4 * D;
    if ((rc = launch_miss_system<1>(pl, pl->opB.d(), E, D, C, Ccov, pl->mZ.d(), pl->mcov.d(), st))) return rc;
    if ((rc = launch_miss_native(pl, A, dtype, D, C, Ccov, out, st))) return rc;
  }
  pl->miss_cov_D = D;
  return TEMX_OK;
}

// ---- latitude-bin form (kernels_bin.hpp, bin_tables.hpp): tables, the binned TEM run and the binned operator ---------
// configurations the binned form serves (checked at temx_plan_configure and again before every binned run)
static int bin_check(const temx_plan* pl) {
  if (pl->K > 64) return fail(TEMX_EUNSUPPORTED, "latitude bins: L = %d, this version supports L <= 63", pl->L);
  if (pl->weighted) return fail(TEMX_EUNSUPPORTED, "latitude bins are not available on a weights-mode plan");
  if (pl->finalized && pl->rank < pl->K)
    return fail(TEMX_EUNSUPPORTED, "latitude bins: the plan was finalised through the pseudo-inverse (rank %d < K = %d; "
                                   "fewer distinct latitudes than harmonics)", pl->rank, pl->K);
  if (miss_mode(pl)) return fail(TEMX_EUNSUPPORTED, "latitude bins are not available in missing-value mode (TEMX_OPT_MISSING = 1)");
  return TEMX_OK;
}

// Built at the first binned temx_plan_set_tem / operator call and again after a change of B or of the plan's basis: the
// sorted rows and chunks, the coefficient tables and the two basis changes
static int bin_setup(temx_plan* pl) {
  if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
  if (int rc = bin_check(pl)) return rc;
  const int B = pl->opt_lat_bins, K = pl->K;
  if (pl->bin_built == B) return TEMX_OK;
  const int J = bin_degree(pl->L, B), KP = (K + 15) / 16 * 16;
  if (J == 0) return fail(TEMX_EINVAL, "TEMX_OPT_LAT_BINS: (L, B) = (%d, %d) is not served", pl->L, B);
  BinRows br;
  if (!build_bin_rows(pl->h_lat.data(), pl->N, B, br))
    return fail(TEMX_EINVAL, "latitude bins: the native latitudes must be finite and lie in [-90, 90] degrees");
  int rc;
  if ((rc = upload(pl->bin_rows, br.rows))) return rc;
  if ((rc = upload(pl->bin_s, br.s))) return rc;
  if ((rc = upload(pl->bin_chunk, br.chunk))) return rc;
  if ((rc = upload(pl->bin_c0, br.bin_chunk0))) return rc;
  if ((rc = upload(pl->bin_a, bin_coefficients(pl->L, B, J, KP)))) return rc;
  std::vector<double> TT((size_t)2 * KP * KP, 0.0);
  for (int l = 0; l < K; ++l)
    for (int j = 0; j < K; ++j) {
      const double t = pl->qbasis ? pl->h_T[(size_t)l * K + j] : (l == j ? 1.0 : 0.0);   // Q_j = sum_l Y_l T[l][j]
      TT[(size_t)j * KP + l] = t;                          // sums: B_Q[j] = sum_l T[l][j] B_Y[l]
      TT[(size_t)KP * KP + (size_t)l * KP + j] = t;        // coefficients: c_Y[l] = sum_j T[l][j] c_Q[j]
    }
  if ((rc = upload(pl->bin_T, TT))) return rc;
  pl->bin_J = J;
  pl->bin_KP = KP;
  pl->bin_nchunk = br.nchunk();
  pl->bin_built = B;
  return TEMX_OK;
}

// workspace of a binned run over D columns of NF fields; TEMX_ENOMEM with the byte count when it does not fit
static int bin_workspace(temx_plan* pl, int64_t D, int NF) {
  const int64_t Dpad = (D + 63) / 64 * 64;
  const size_t need_cm = (size_t)pl->bin_nchunk * NF * pl->bin_J * Dpad * 8;
  const size_t need_z = (size_t)pl->opt_lat_bins * NF * pl->bin_J * Dpad * 8;
  const size_t need_cy = (size_t)NF * pl->K * D * 8;
  const size_t need_p = (size_t)BIN_SLABS * NF * pl->K * D * 8;
  size_t more = 0;
  const DevBuf* bufs[4] = {&pl->bin_cm, &pl->bin_z, &pl->bin_cy, &pl->partial};
  const size_t needs[4] = {need_cm, need_z, need_cy, need_p};
  for (int i = 0; i < 4; ++i)
    if (bufs[i]->bytes < needs[i]) more += needs[i];
  size_t fr = 0, tot = 0;
  if (more && hipMemGetInfo(&fr, &tot) == hipSuccess && more > fr)
    return fail(TEMX_ENOMEM, "latitude bins: the workspace of the binned sweeps needs %zu more bytes (chunk moments %zu, series %zu), "
                             "%zu are free; process the snapshots in smaller blocks", more, need_cm, need_z, fr);
  int rc;
  if ((rc = pl->bin_cm.ensure(need_cm))) return rc;
  if ((rc = pl->bin_z.ensure(need_z))) return rc;
  if ((rc = pl->bin_cy.ensure(need_cy))) return rc;
  return pl->partial.ensure(need_p);
}

static int bin_set_tem(temx_plan* pl) {
  if (int rc = bin_setup(pl)) return rc;
  return bin_workspace(pl, pl->D, 4);
}

// chunk moments of NF fields -> raw sums B[NF][K][D] in the plan's projection basis
static int bin_contract(temx_plan* pl, int NF, int64_t D, double* B, hipStream_t st) {
  const int Dw = (int)((D + 63) / 64);
  const int* c0 = static_cast<const int*>(pl->bin_c0.p);
  const dim3 grid((unsigned)Dw, (unsigned)NF, BIN_SLABS);
  int rc = dispatch(BinKPValues{}, pl->bin_KP, [&](auto kp) {
    return launch<bin_contract_kernel<decltype(kp)::value>>(grid, dim3(64), 0, st, pl->bin_cm.d(), NF, pl->bin_J, D, Dw,
                                                            pl->opt_lat_bins, pl->K, c0, pl->bin_a.d(), pl->partial.d());
  });
  if (rc) return rc;
  if ((rc = launch_reduce(pl, pl->partial.d(), BIN_SLABS, (int64_t)NF * pl->K * D, B, st))) return rc;
  if (!pl->qbasis) return TEMX_OK;
  const dim3 gb((unsigned)Dw, (unsigned)NF);
  return dispatch(BinKPValues{}, pl->bin_KP, [&](auto kp) {
    return launch<bin_basis_kernel<decltype(kp)::value>>(gb, dim3(64), 0, st, B, (int64_t)pl->K, pl->bin_T.d(), pl->K, D, B,
                                                         (int64_t)pl->K);
  });
}

// coefficients C[NF][K4][D] in the plan's basis -> the per-bin Chebyshev series z[B][NF][J][Dpad] of the native means
static int bin_synth(temx_plan* pl, int NF, int64_t D, const double* C, hipStream_t st) {
  const int Dw = (int)((D + 63) / 64);
  const int* c0 = static_cast<const int*>(pl->bin_c0.p);
  const double* Tc = pl->bin_T.d() + (size_t)pl->bin_KP * pl->bin_KP;
  const dim3 gb((unsigned)Dw, (unsigned)NF), grid((unsigned)Dw, (unsigned)NF, BIN_SLABS);
  return dispatch(BinKPValues{}, pl->bin_KP, [&](auto kp) {
    constexpr int KP = decltype(kp)::value;
    hipLaunchKernelGGL(bin_basis_kernel<KP>, gb, dim3(64), 0, st, C, (int64_t)pl->K4, Tc, pl->K, D, pl->bin_cy.d(),
        (int64_t)pl->K);
    return launch<bin_synth_kernel<KP>>(grid, dim3(64), 0, st, pl->bin_cy.d(), NF, pl->bin_J, D, Dw, pl->opt_lat_bins,
        pl->K, c0, pl->bin_a.d(), pl->bin_z.d());
  });
}

// temx_tem_run with latitude bins: two reads of the four fields; B4, C4, the zonal means and the validity flags are
// left as the generic two-pass stages leave them, so that the eddies and the tracers run their own kernels afterwards
static int bin_tem_run(temx_plan* pl, const FieldPtrs<4>& fp, int dtype, double* results, double* zonal, hipStream_t st) {
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  int rc;
  if ((rc = bin_setup(pl))) return rc;
  const int64_t D = pl->D;
  if ((rc = bin_workspace(pl, D, 4))) return rc;
  set_tail(pl, 0, pl->nt);
  pl->op_valid = pl->os_valid = pl->c4_valid = pl->tq_valid = false;
  TimedLaunch tl{};
  time_begin(pl, 0, st, tl);
  rc = launch_bin_moments<4>(pl, fp, dtype, D, pl->colscale.d(), 2, st);
  time_end(pl, 0, st, tl);
  if (rc) return rc;
  if ((rc = bin_contract(pl, 4, D, pl->B4.d(), st))) return rc;
  // C = G^-1 B4 and the four zonal means ub vb thetab wapb -> zb[0..3]
  if ((rc = launch_solve(pl, pl->B4.d(), 4, D, pl->C4.d(), pl->zb.d(), st))) return rc;
  pl->c4_valid = true;
  if ((rc = bin_synth(pl, 4, D, pl->C4.d(), st))) return rc;
  const int Dw = (int)((D + 63) / 64);
  const dim3 grid = bin_sweep_grid(pl, D);
  const int4* ch = static_cast<const int4*>(pl->bin_chunk.p);
  const int* rows = static_cast<const int*>(pl->bin_rows.p);
  TimedLaunch tl2{};
  time_begin(pl, 1, st, tl2);
  rc = by_dtype(dtype, [&](auto t) {
    return dispatch(BinJValues{}, pl->bin_J, [&](auto j) {
      return launch<bin_eddy_moments_kernel<typename decltype(t)::type, decltype(j)::value>>(
          grid, dim3(256), 0, st, fp, D, Dw, ch, rows, pl->bin_s.d(), pl->colscale.d(), pl->bin_z.d(), pl->bin_cm.d());
    });
  });
  time_end(pl, 1, st, tl2);
  if (rc) return rc;
  if ((rc = bin_contract(pl, 3, D, pl->B3.d(), st))) return rc;
  return tem_stage3_impl(pl, pl->B3.d(), results, zonal, st);
}

// temx_project with latitude bins
static int bin_project_op(temx_plan* pl, const void* A, int dtype, int64_t D, double* B, hipStream_t st) {
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  int rc;
  if ((rc = bin_setup(pl))) return rc;
  if ((rc = bin_workspace(pl, D, 1))) return rc;
  FieldPtrs<1> fp;
  fp.p[0] = A;
  if ((rc = launch_bin_moments<1>(pl, fp, dtype, D, nullptr, -1, st))) return rc;
  return bin_contract(pl, 1, D, B, st);
}

// temx_zonal_mean with latitude bins: the binned projection, the plan's solve, and for the native mean the per-bin
// series evaluated at every column
static int bin_zonal_mean(temx_plan* pl, const void* A, int dtype, int64_t D, double* out, int native, hipStream_t st) {
  if (D < 1 || D >= ((int64_t)1 << 28)) return fail(TEMX_EINVAL, "D must be in [1, 2^28)");
  HIPCHK(hipSetDevice(pl->device));
  int rc;
  if ((rc = pl->opB.ensure((size_t)pl->K * D * 8))) return rc;
  if ((rc = bin_project_op(pl, A, dtype, D, pl->opB.d(), st))) return rc;
  if (!native) return launch_solve(pl, pl->opB.d(), 1, D, nullptr, out, st);
  if ((rc = pl->opC.ensure((size_t)pl->K4 * D * 8))) return rc;
  if ((rc = launch_solve(pl, pl->opB.d(), 1, D, pl->opC.d(), nullptr, st))) return rc;
  if ((rc = bin_synth(pl, 1, D, pl->opC.d(), st))) return rc;
  const int Dw = (int)((D + 63) / 64);
  const int4* ch = static_cast<const int4*>(pl->bin_chunk.p);
  const int* rows = static_cast<const int*>(pl->bin_rows.p);
  return dispatch(BinJValues{}, pl->bin_J, [&](auto j) {
    return launch<bin_native_kernel<decltype(j)::value>>(bin_sweep_grid(pl, D), dim3(256), 0, st, D, Dw, ch, rows,
        pl->bin_s.d(), pl->bin_z.d(), out);
  });
}

int temx_tem_run(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap,
                 int dtype, double* results, double* zonal, void* stream) try {
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (miss_mode(pl)) {
    if (!ua || !va || !ta || !wap || !results) return fail(TEMX_EINVAL, "null argument");
    HIPCHK(hipSetDevice(pl->device));
    return miss_tem_run(pl, four(ua, va, ta, wap), dtype, results, zonal, S_(stream));
  }
  if (bin_mode(pl)) {
    if (!ua || !va || !ta || !wap || !results) return fail(TEMX_EINVAL, "null argument");
    HIPCHK(hipSetDevice(pl->device));
    return bin_tem_run(pl, four(ua, va, ta, wap), dtype, results, zonal, S_(stream));
  }
  if (os_active(pl, dtype)) {
    if ((rc = os_ready(pl))) return rc;
    if (!ua || !va || !ta || !wap || !results) return fail(TEMX_EINVAL, "null argument");
    if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
    HIPCHK(hipSetDevice(pl->device));
    return tem_run_os(pl, four(ua, va, ta, wap), dtype, results, zonal, stream);
  }
  if ((rc = temx_tem_stage1(pl, ua, va, ta, wap, dtype, pl->B4.d(), stream))) return rc;
  if (temx_plan_one_pass(pl))
    rc = temx_tem_stage2_from_sums(pl, pl->B4.d(), pl->B3.d(), stream);
  else
    rc = temx_tem_stage2(pl, ua, va, ta, wap, dtype, pl->B4.d(), pl->B3.d(), stream);
  if (rc) return rc;
  return temx_tem_stage3(pl, pl->B3.d(), results, zonal, stream);
} TEMX_CATCH

int temx_tem_eddy(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap,
                  int dtype, double* const* eddy_ptrs_host, void* stream) try {
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!ua || !va || !ta || !wap || !eddy_ptrs_host) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  if (!tail_is_whole(pl)) return fail(TEMX_ESTATE, "the plan holds the coefficients of a time slice (temx_tem_os_tail), not of the whole run");
  EddyOut eo;
  for (int i = 0; i < TEMX_NEDDY; ++i) eo.p[i] = eddy_ptrs_host[i];
  if (miss_mode(pl)) {
    if (!pl->miss_valid) return fail(TEMX_ESTATE, "missing-value mode: the eddies need a masked temx_tem_run on this plan first");
    return launch_miss_eddy_native(pl, four(ua, va, ta, wap), dtype, 0, pl->N, eo, S_(stream));
  }
  if (unfused_stage2(pl)) {
    if ((rc = ensure_xb(pl, S_(stream)))) return rc;
    return launch_eddy_from_xbar(pl, four(ua, va, ta, wap), dtype, native_means(pl, 0, 1, 2, 3),
                                 pl->colscale.d(), eo, S_(stream));
  }
  return run_eddy<0>(pl, four(ua, va, ta, wap), dtype, pl->C4.d(), nullptr, &eo, S_(stream));
} TEMX_CATCH

int temx_tem_eddy_rows(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap,
                       int dtype, int64_t row0, int64_t nrows, double* const* eddy_ptrs_host, void* stream) try {
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!ua || !va || !ta || !wap || !eddy_ptrs_host) return fail(TEMX_EINVAL, "null argument");
  if (row0 < 0 || nrows < 1 || row0 + nrows > pl->N || (row0 & 15))
    return fail(TEMX_EINVAL, "row range [%lld, %lld) must lie inside the grid and start at a multiple of 16",
                (long long)row0, (long long)(row0 + nrows));
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  HIPCHK(hipSetDevice(pl->device));
  if (!tail_is_whole(pl)) return fail(TEMX_ESTATE, "the plan holds the coefficients of a time slice (temx_tem_os_tail), not of the whole run");
  hipStream_t st = S_(stream);
  if (miss_mode(pl)) {
    if (!pl->miss_valid) return fail(TEMX_ESTATE, "missing-value mode: the eddies need a masked temx_tem_run on this plan first");
    EddyOut eo;
    for (int i = 0; i < TEMX_NEDDY; ++i) eo.p[i] = eddy_ptrs_host[i];
    return launch_miss_eddy_native(pl, four(ua, va, ta, wap), dtype, row0, nrows, eo, st);
  }
  const int64_t D = pl->D, nd = nrows * D;
  // native zonal means of the rows (coefficients of the last temx_tem_stage2), then elementwise eddies
  DevBuf& ws = pl->opC;                       // operator-API workspace doubles as the row-chunk buffer
  if ((rc = ws.ensure((size_t)4 * nd * 8))) return rc;
  FieldPtrs<4> xb, fp;
  const void* src[4] = {ua, va, ta, wap};
  const size_t es = dtype == TEMX_F64 ? 8 : 4;
  for (int f = 0; f < 4; ++f) {
    double* o = ws.d() + (int64_t)f * nd;
    if ((rc = launch_recon(pl, D, pl->C4.d() + (int64_t)f * pl->K4 * D, o, st, row0, nrows))) return rc;
    xb.p[f] = o;
    fp.p[f] = static_cast<const char*>(src[f]) + (size_t)row0 * D * es;
  }
  EddyOut eo;
  for (int i = 0; i < TEMX_NEDDY; ++i) eo.p[i] = eddy_ptrs_host[i];
  return launch_eddy_from_xbar(pl, fp, dtype, xb, pl->colscale.d(), eo, st, nrows);
} TEMX_CATCH

// ---- tracer TEM -----------------------------------------------------------------------------------
static int tracer_ws(temx_plan* pl) {
  const TracerWs w = tracer_ws_layout(tem_dims(pl), pl->sp_proj1, pl->sp_cproj1);
  int rc;
  if ((rc = pl->Bq.ensure(w.Bq))) return rc;
  if ((rc = pl->Bq2.ensure(w.Bq2))) return rc;
  if ((rc = pl->Ct.ensure(w.Ct))) return rc;
  if ((rc = pl->tz.ensure(w.tz))) return rc;
  return pl->partial.ensure(w.partial);
}

int temx_tracer_stage1(temx_plan* pl, const void* q, int dtype, double* Bq, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracer_stage1");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tracer_stage1");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!q || !Bq) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  if ((rc = tracer_ws(pl))) return rc;
  FieldPtrs<1> fp;
  fp.p[0] = q;
  if (pl->large) return project_all<1>(pl, fp, dtype, pl->D, nullptr, -1, pl->sp_proj1, Bq, S_(stream));
  const bool sp1 = sym_project(pl, 1);
  const Split& sp = pl->cls ? pl->sp_cproj1 : (sp1 ? pl->sp_sproj1 : pl->sp_proj1);
  rc = pl->cls ? launch_project_cls<1>(pl, fp, dtype, pl->D, nullptr, -1, pl->partial.d(), sp, S_(stream))
       : sp1   ? launch_project_sym<1>(pl, fp, dtype, pl->D, nullptr, -1, pl->partial.d(), sp, S_(stream))
               : launch_project<1>(pl, fp, dtype, pl->D, nullptr, -1, pl->partial.d(), sp, S_(stream));
  if (rc) return rc;
  return launch_reduce(pl, pl->partial.d(), sp.nsplit, (int64_t)pl->K * pl->D, Bq, S_(stream));
} TEMX_CATCH

int temx_tracer_stage2(temx_plan* pl, const void* q, const void* va, const void* wap, int dtype,
                       const double* Bq, double* Bq2, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracer_stage2");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tracer_stage2");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!q || !va || !wap || !Bq || !Bq2) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  if (!tail_is_whole(pl)) return fail(TEMX_ESTATE, "the plan holds the coefficients of a time slice (temx_tem_os_tail), not of the whole run");
  if ((rc = tracer_ws(pl))) return rc;
  hipStream_t st = S_(stream);
  const size_t slab = (size_t)pl->K4 * pl->D * 8;
  // coefficients: Ct = (C_q, C_v, C_w); qb -> tz[0]
  if ((rc = launch_solve(pl, Bq, 1, pl->D, pl->Ct.d(), pl->tz.d(), st))) return rc;
  if (unfused_stage2(pl)) {   // q' v' and q' omega' from the native means of the last temx_tem_stage2
    if ((rc = ensure_xb(pl, st))) return rc;
    const int64_t nd = pl->N * pl->D;
    if ((rc = launch_recon(pl, pl->D, pl->Ct.d(), pl->XB.d() + 4 * nd, st))) return rc;
    EddyOut eo{};
    eo.p[4] = pl->P3.d();
    eo.p[5] = pl->P3.d() + nd;
    if ((rc = launch_eddy_from_xbar(pl, four(q, va, va, wap), dtype, native_means(pl, 4, 1, 1, 3), nullptr, eo, st)))
      return rc;
    for (int i = 0; i < 2; ++i) {
      FieldPtrs<1> f1;
      f1.p[0] = eo.p[4 + i];
      if ((rc = project_all<1>(pl, f1, TEMX_F64, pl->D, nullptr, -1, pl->sp_proj1, Bq2 + (int64_t)i * pl->K * pl->D, st)))
        return rc;
    }
    return TEMX_OK;
  }
  HIPCHK(hipMemcpyAsync((char*)pl->Ct.p + slab, (char*)pl->C4.p + slab, slab, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync((char*)pl->Ct.p + 2 * slab, (char*)pl->C4.p + 3 * slab, slab, hipMemcpyDeviceToDevice, st));
  if ((rc = run_eddy<1>(pl, four(q, va, wap, nullptr), dtype, pl->Ct.d(), pl->partial.d(), nullptr, st))) return rc;
  return launch_reduce(pl, pl->partial.d(), eddy_slabs(pl), (int64_t)2 * pl->K * pl->D, Bq2, st);
} TEMX_CATCH

int temx_tracer_stage3(temx_plan* pl, const double* Bq2, double* tres, double* tzon, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracer_stage3");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tracer_stage3");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!Bq2 || !tres) return fail(TEMX_EINVAL, "null argument");
  if (!pl->tz.p) return fail(TEMX_ESTATE, "temx_tracer_stage2 has not been called");
  if (!tail_is_whole(pl)) return fail(TEMX_ESTATE, "the plan holds the zonal means of a time slice (temx_tem_os_tail)");
  HIPCHK(hipSetDevice(pl->device));
  return tracer_stage3_impl(pl, Bq2, tres, tzon, S_(stream));
} TEMX_CATCH

static int tracer_stage3_impl(temx_plan* pl, const double* Bq2, double* tres, double* tzon, hipStream_t st) {
  int rc;
  const int64_t Dt = pl->tD;
  const int64_t MD = (int64_t)pl->M * Dt;
  if ((rc = launch_solve(pl, Bq2, 2, Dt, nullptr, pl->tz.d() + MD, st))) return rc;   // qpvpb, qpwappb
  EpiTables tb{pl->p.d(), pl->pg.d(), pl->lg.d(), pl->coslat.d(), pl->fcor.d()};
  hipLaunchKernelGGL(tracer_epilogue_kernel, dim3((unsigned)((MD + 255) / 256)), dim3(256), 0, st, pl->zb.d(),
                     pl->tz.d(), pl->M, pl->nlev, pl->tnt, tb, pl->p0, tres, tzon);
  HIPCHK(hipGetLastError());
  return TEMX_OK;
}

// the one-pass tracer stages pair q's class sums with the v, omega class sums (csum: stage 1) and with the v,
// omega coefficients (C4: stage 2) of the latest TEM run; both must describe the same fields
static inline bool tracer_one_pass(const temx_plan* pl) { return pl->cls && pl->onepass && pl->op_valid; }

int temx_tracer_stage1_sums(temx_plan* pl, const void* q, const void* va, const void* wap, int dtype,
                            double* Bq, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracer_stage1_sums");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tracer_stage1_sums");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!q || !va || !wap || !Bq) return fail(TEMX_EINVAL, "null argument");
  if (!tracer_one_pass(pl))
    return fail(TEMX_ESTATE, "needs the one-pass class path and the class sums of a TEM run on this plan "
                             "(temx_plan_one_pass, temx_tem_stage1)");
  HIPCHK(hipSetDevice(pl->device));
  if ((rc = tracer_ws(pl))) return rc;
  hipStream_t st = S_(stream);
  const Split& sp = pl->sp_cproj4;
  const int64_t KD = (int64_t)pl->K * pl->D;
  if ((rc = pl->csq.ensure((size_t)pl->cgroups * sp.ndt * 2 * 64 * 8))) return rc;
  if ((rc = pl->Pq2.ensure((size_t)2 * KD * 8))) return rc;
  pl->tq_valid = false;
  // one read of (q, v, omega): 3 slabs per split -- q, then the co-moments of q v and q omega
  if ((rc = launch_sweep_op<1>(pl, four(q, va, wap, nullptr), dtype, pl->partial.d(), sp, st))) return rc;
  if ((rc = launch_reduce(pl, pl->partial.d(), sp.nsplit, KD, Bq, st, 3 * KD))) return rc;
  if ((rc = launch_reduce(pl, pl->partial.d() + KD, sp.nsplit, 2 * KD, pl->Pq2.d(), st, 3 * KD))) return rc;
  pl->tq_valid = true;
  return TEMX_OK;
} TEMX_CATCH

int temx_tracer_stage2_from_sums(temx_plan* pl, const double* Bq, double* Bq2, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracer_stage2_from_sums");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tracer_stage2_from_sums");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!Bq || !Bq2) return fail(TEMX_EINVAL, "null argument");
  if (tracer_one_pass(pl) && !pl->c4_valid)
    return fail(TEMX_ESTATE, "temx_tem_stage1 ran on new fields but no temx_tem_stage2 since: the v, omega "
                             "coefficients belong to the previous fields");
  if (!tracer_one_pass(pl) || !pl->tq_valid)
    return fail(TEMX_ESTATE, "no tracer class sums: temx_tracer_stage1_sums must precede temx_tracer_stage2_from_sums");
  HIPCHK(hipSetDevice(pl->device));
  if (!tail_is_whole(pl)) return fail(TEMX_ESTATE, "the plan holds the coefficients of a time slice (temx_tem_os_tail), not of the whole run");
  hipStream_t st = S_(stream);
  const size_t slab = (size_t)pl->K4 * pl->D * 8;
  // coefficients: Ct = (C_q, C_v, C_w); qb -> tz[0]
  if ((rc = launch_solve(pl, Bq, 1, pl->D, pl->Ct.d(), pl->tz.d(), st))) return rc;
  HIPCHK(hipMemcpyAsync((char*)pl->Ct.p + slab, (char*)pl->C4.p + slab, slab, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync((char*)pl->Ct.p + 2 * slab, (char*)pl->C4.p + 3 * slab, slab, hipMemcpyDeviceToDevice, st));
  if ((rc = launch_flux_cls<1>(pl, pl->Ct.d(), pl->partial.d(), pl->sp_cflux, st))) return rc;
  // Bq2 = (projected co-moments of q v, q omega from the sweep) + (projected n (m_q - qb)(m_v - vb) terms)
  return launch_reduce(pl, pl->partial.d(), pl->sp_cflux.nsplit, (int64_t)2 * pl->K * pl->D, Bq2, st, -1,
                       pl->Pq2.d());
} TEMX_CATCH

// TEM stage 1 and the tracer's one-pass stage 1 in ONE sweep over (u, v, T, omega, q): the fields are read once
// for both (40 B per grid point instead of 32 + 24).  State afterwards: as after temx_tem_stage1 followed by
// temx_tracer_stage1_sums.
int temx_tem_tracer_stage1(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap,
                           const void* q, int dtype, double* B4, double* Bq, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_tracer_stage1");
  if (pl && bin_refused(pl)) return bin_refuse("temx_tem_tracer_stage1");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!ua || !va || !ta || !wap || !q || !B4 || !Bq) return fail(TEMX_EINVAL, "null argument");
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  if (!(pl->cls && pl->onepass) || pl->large)
    return fail(TEMX_ESTATE, "the fused TEM + tracer sweep needs the one-pass class path (temx_plan_one_pass)");
  HIPCHK(hipSetDevice(pl->device));
  if ((rc = tracer_ws(pl))) return rc;
  hipStream_t st = S_(stream);
  const Split& sp = pl->sp_copw;
  const int64_t KD = (int64_t)pl->K * pl->D;
  if ((rc = pl->csq.ensure((size_t)pl->cgroups * sp.ndt * 2 * 64 * 8))) return rc;
  if ((rc = pl->Pq2.ensure((size_t)2 * KD * 8))) return rc;
  if ((rc = pl->partial.ensure(tem_tracer_stage1_partial(tem_dims(pl), sp)))) return rc;
  set_tail(pl, 0, pl->nt);
  pl->op_valid = pl->c4_valid = pl->tq_valid = pl->os_valid = false;
  FieldPtrs<5> fp;
  fp.p[0] = ua; fp.p[1] = va; fp.p[2] = ta; fp.p[3] = wap; fp.p[4] = q;
  TimedLaunch tl{};
  time_begin(pl, 0, st, tl);
  rc = dtype == TEMX_F64 ? launch_sweep_opw2_t<double>(pl, fp, pl->partial.d(), sp, st)
                         : launch_sweep_opw2_t<float>(pl, fp, pl->partial.d(), sp, st);
  time_end(pl, 0, st, tl);
  if (rc) return rc;
  // 10 slabs per split: u v theta omega | q | u v, u omega, v theta | q v, q omega
  const double* P = pl->partial.d();
  if ((rc = launch_reduce(pl, P, sp.nsplit, 4 * KD, B4, st, 10 * KD))) return rc;
  if ((rc = launch_reduce(pl, P + 4 * KD, sp.nsplit, KD, Bq, st, 10 * KD))) return rc;
  if ((rc = launch_reduce(pl, P + 5 * KD, sp.nsplit, 3 * KD, pl->Pq.d(), st, 10 * KD))) return rc;
  if ((rc = launch_reduce(pl, P + 8 * KD, sp.nsplit, 2 * KD, pl->Pq2.d(), st, 10 * KD))) return rc;
  pl->op_valid = true;
  pl->tq_valid = true;
  return TEMX_OK;
} TEMX_CATCH

int temx_tem_tracer_run(temx_plan* pl, const void* ua, const void* va, const void* ta, const void* wap,
                        const void* q, int dtype, double* results, double* zonal, double* tres, double* tzon,
                        void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tem_tracer_run");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!q || !tres) return fail(TEMX_EINVAL, "null argument");
  // any other path -- or the single-sweep forms, which beat the fused class-sum sweep -- : the two runs one after the other
  if (!(pl->cls && pl->onepass) || pl->large || os_active(pl, dtype)) {
    if ((rc = temx_tem_run(pl, ua, va, ta, wap, dtype, results, zonal, stream))) return rc;
    return temx_tracer_run(pl, q, va, wap, dtype, tres, tzon, stream);
  }
  if ((rc = tracer_ws(pl))) return rc;
  if ((rc = temx_tem_tracer_stage1(pl, ua, va, ta, wap, q, dtype, pl->B4.d(), pl->Bq.d(), stream))) return rc;
  if ((rc = temx_tem_stage2_from_sums(pl, pl->B4.d(), pl->B3.d(), stream))) return rc;
  if ((rc = temx_tem_stage3(pl, pl->B3.d(), results, zonal, stream))) return rc;
  if ((rc = temx_tracer_stage2_from_sums(pl, pl->Bq.d(), pl->Bq2.d(), stream))) return rc;
  return temx_tracer_stage3(pl, pl->Bq2.d(), tres, tzon, stream);
} TEMX_CATCH

int temx_tracer_run(temx_plan* pl, const void* q, const void* va, const void* wap, int dtype,
                    double* tres, double* tzon, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracer_run");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (pl->os_valid && pl->c4_valid && tail_is_whole(pl) && os_active(pl, dtype)) {   // after a single-sweep TEM run: the tracer's single sweep
    if (!q || !va || !wap || !tres) return fail(TEMX_EINVAL, "null argument");
    if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
    HIPCHK(hipSetDevice(pl->device));
    const void* qs[1] = {q};
    double* tr[1] = {tres};
    double* tz[1] = {tzon};
    return tracer_run_os(pl, 1, qs, va, wap, dtype, tr, tz, stream);
  }
  if ((rc = tracer_ws(pl))) return rc;
  BinPass through_stages(pl);      // latitude bins: the tracer's stages are the plan's own two-pass kernels, unchanged
  // The one-pass form reads (q, v, omega) once instead of q + (q, v, omega), but its sweep shares a SIMD
  // with fewer waves than the two-pass kernels: measured on ne120 x 72 x 30 it is no faster (10.2 ms
  // against 9.6 ms), so the two-pass stages stay the default and TEMX_TRACER_ONE_PASS=1 selects it.
  if (tracer_one_pass_wanted(pl) && tracer_one_pass(pl)) {
    if ((rc = temx_tracer_stage1_sums(pl, q, va, wap, dtype, pl->Bq.d(), stream))) return rc;
    if ((rc = temx_tracer_stage2_from_sums(pl, pl->Bq.d(), pl->Bq2.d(), stream))) return rc;
    return temx_tracer_stage3(pl, pl->Bq2.d(), tres, tzon, stream);
  }
  if ((rc = temx_tracer_stage1(pl, q, dtype, pl->Bq.d(), stream))) return rc;
  if ((rc = temx_tracer_stage2(pl, q, va, wap, dtype, pl->Bq.d(), pl->Bq2.d(), stream))) return rc;
  return temx_tracer_stage3(pl, pl->Bq2.d(), tres, tzon, stream);
} TEMX_CATCH

// nq tracers of one TEM run (tem_diagnostics.py:281-301 takes a list): after a single-sweep TEM run they are swept
// in PAIRS -- (q1, q2, v, omega) read once: the traffic of the TEM sweep for two tracers instead of 3/4 of it for each
// -- and a last odd one alone; on any other path one temx_tracer_run after the other.
int temx_tracers_run(temx_plan* pl, int nq, const void* const* q_host, const void* va, const void* wap, int dtype,
                     double* const* tres_host, double* const* tzon_host, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracers_run");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (nq < 1 || !q_host || !tres_host) return fail(TEMX_EINVAL, "bad argument");
  for (int i = 0; i < nq; ++i)
    if (!q_host[i] || !tres_host[i]) return fail(TEMX_EINVAL, "null argument");
  const bool os = pl->os_valid && pl->c4_valid && tail_is_whole(pl) && os_active(pl, dtype) && !pl->os_tile && !pl->osc_lds &&
                  (dtype == TEMX_F64 || dtype == TEMX_F32);
  int i = 0;
  if (os) {
    if (!va || !wap) return fail(TEMX_EINVAL, "null argument");
    if ((rc = os_ready(pl))) return rc;
    HIPCHK(hipSetDevice(pl->device));
    for (; i + 1 < nq; i += 2)
      if ((rc = tracer_run_os(pl, 2, q_host + i, va, wap, dtype, tres_host + i, tzon_host ? tzon_host + i : nullptr, stream))) return rc;
  }
  for (; i < nq; ++i)
    if ((rc = temx_tracer_run(pl, q_host[i], va, wap, dtype, tres_host[i], tzon_host ? tzon_host[i] : nullptr, stream))) return rc;
  return TEMX_OK;
} TEMX_CATCH

int temx_tracer_eddy(temx_plan* pl, const void* q, const void* va, const void* wap, int dtype,
                     double* const* ptrs3_host, void* stream) try {
  if (pl && miss_mode(pl)) return miss_refuse("temx_tracer_eddy");
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!q || !va || !wap || !ptrs3_host) return fail(TEMX_EINVAL, "null argument");
  if (!pl->Ct.p) return fail(TEMX_ESTATE, "temx_tracer_stage2 has not been called");
  HIPCHK(hipSetDevice(pl->device));
  if (!tail_is_whole(pl)) return fail(TEMX_ESTATE, "the plan holds the coefficients of a time slice (temx_tem_os_tail), not of the whole run");
  EddyOut eo{};
  eo.p[0] = ptrs3_host[0];
  eo.p[4] = ptrs3_host[1];
  eo.p[5] = ptrs3_host[2];
  if (unfused_stage2(pl)) {
    if (!pl->xb_valid) return fail(TEMX_ESTATE, "temx_tracer_stage2 has not been called since the last TEM run");
    return launch_eddy_from_xbar(pl, four(q, va, va, wap), dtype, native_means(pl, 4, 1, 1, 3), nullptr, eo,
                                 S_(stream));
  }
  return run_eddy<1>(pl, four(q, va, wap, nullptr), dtype, pl->Ct.d(), nullptr, &eo, S_(stream));
} TEMX_CATCH

int temx_status(temx_plan* pl, int* nonfinite, void* stream) try {
  if (!pl || !nonfinite) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(pl->device));
  HIPCHK(hipStreamSynchronize(S_(stream)));
  int fw[2] = {0, 0};
  HIPCHK(hipMemcpy(fw, pl->flag.p, sizeof(fw), hipMemcpyDeviceToHost));
  const int f = fw[0];
  *nonfinite = miss_mode(pl) ? 0 : f;     // missing-value mode: non-finite input is data, not an error
  if (f || fw[1]) {
    const int zero[2] = {0, 0};
    HIPCHK(hipMemcpy(pl->flag.p, zero, sizeof(zero), hipMemcpyHostToDevice));
  }
  if (fw[1])   // (kernels_op2.hpp, sweep_osr_kernel<SYNC = 1>: a wave gave up waiting; the results of that run are not valid)
    return fail(TEMX_EINTERNAL, "single sweep: the hand-over of the class sums between the waves of a workgroup timed out "
                "(code %d); results of the runs since the last temx_status are invalid. TEMX_OS_SYNC=barrier selects the barrier form", fw[1]);
  return TEMX_OK;
} TEMX_CATCH

// ---- measurement helpers -------------------------------------------------------------------------
int temx_synth_fields(int device, int64_t ncol, int nlev, int64_t nt, int64_t t0, const double* lat_deg,
                      const double* lon_deg, const double* plev_hpa, int dtype, uint64_t seed, void* ua,
                      void* va, void* ta, void* wap, void* stream) try {
  if (!lat_deg || !lon_deg || !plev_hpa || !ua || !va || !ta || !wap) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(device));
  dim3 grid(256 * 16), block(256);
  if (dtype == TEMX_F64) {
    hipLaunchKernelGGL(synth_kernel<double>, grid, block, 0, S_(stream), ncol, nlev, nt, t0, lat_deg, lon_deg,
                       plev_hpa, seed, (double*)ua, (double*)va, (double*)ta, (double*)wap);
  } else if (dtype == TEMX_F32) {
    hipLaunchKernelGGL(synth_kernel<float>, grid, block, 0, S_(stream), ncol, nlev, nt, t0, lat_deg, lon_deg,
                       plev_hpa, seed, (float*)ua, (float*)va, (float*)ta, (float*)wap);
  } else {
    return bad_dtype();
  }
  HIPCHK(hipGetLastError());
  return TEMX_OK;
} TEMX_CATCH

int temx_mfma_f64_peak(int device, int iters, double* tflops_out) try {
  if (!tflops_out || iters < 1) return fail(TEMX_EINVAL, "bad argument");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  double* sink = nullptr;
  HIPCHK(hipMalloc(&sink, 8));
  const int blocks = prop.multiProcessorCount * 2;  // 8 waves per CU, 2 per SIMD
  hipEvent_t a = nullptr, b = nullptr;
  float ms = 0.f;
  hipError_t e = hipEventCreate(&a);
  if (e == hipSuccess) e = hipEventCreate(&b);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, 0, iters, sink);  // warm-up
    e = hipEventRecord(a, 0);
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, 0, iters, sink);
    e = hipEventRecord(b, 0);
  }
  if (e == hipSuccess) e = hipEventSynchronize(b);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
  if (a) (void)hipEventDestroy(a);
  if (b) (void)hipEventDestroy(b);
  (void)hipFree(sink);
  if (e != hipSuccess) return fail(TEMX_EHIP, "mfma peak benchmark failed: %s", hipGetErrorString(e));
  const double flops = (double)blocks * 4.0 * iters * 8.0 * 512.0;
  *tflops_out = flops / (ms * 1e-3) / 1e12;
  return TEMX_OK;
} TEMX_CATCH

int temx_kernel_timing(temx_plan* pl, int enable) try {
  if (!pl) return fail(TEMX_EINVAL, "null plan");
  HIPCHK(hipSetDevice(pl->device));
  pl->timing = enable != 0;
  for (int w = 0; w < 2; ++w) {
    for (auto& tl : pl->timed[w]) {
      (void)hipEventDestroy(tl.a);
      (void)hipEventDestroy(tl.b);
    }
    pl->timed[w].clear();
  }
  return TEMX_OK;
} TEMX_CATCH

int temx_kernel_timing_read(temx_plan* pl, int which, double* avg_ms, int* launches) try {
  if (!pl || !avg_ms || !launches || which < 0 || which > 1) return fail(TEMX_EINVAL, "bad argument");
  HIPCHK(hipSetDevice(pl->device));
  double tot = 0.0;
  int n = 0;
  for (auto& tl : pl->timed[which]) {
    HIPCHK(hipEventSynchronize(tl.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, tl.a, tl.b));
    tot += ms;
    ++n;
  }
  *avg_ms = n ? tot / n : 0.0;
  *launches = n;
  return TEMX_OK;
} TEMX_CATCH

int temx_selftest_exception(int kind) try {
  if (kind == 0) throw std::bad_alloc();
  if (kind == 1) throw std::runtime_error("self-test");
  if (kind == 2) throw 42;
  return fail(TEMX_EINVAL, "kind must be 0, 1 or 2");
} TEMX_CATCH

// ---- vertical interpolation (include/temx_vert.h) ------------------------------------------------
int temxv_version(void) { return 100; }

// the level tables of a remap on `device`, through the cache of vert_tables; hyam null: no hybrid coefficients
static int vert_tab_on(int device, int nlev, const double* hyam, const double* hybm, int nplev, const double* plev,
                       int method, VertTab* tb) {
  const double* dev = nullptr;
  if (int rc = vert_tables(device, vert_table_host(nlev, hyam, hybm, nplev, plev, method), &dev)) return rc;
  *tb = VertTab{};
  if (hyam) tb->hyam = dev, tb->hybm = dev + nlev, dev += 2 * (size_t)nlev;
  tb->pt = dev, tb->xt = dev + nplev;
  return TEMX_OK;
}

int temxv_interp(int device, int nf, const void* const* src_host, void* const* dst_host, int dtype, int64_t ncol,
                 int nlev, int64_t nt, int nplev, const double* plev_pa_host, int pmode, const double* hyam_host,
                 const double* hybm_host, double p0_hybrid, const void* ps_or_p, int p_dtype, int method, int edge,
                 void* stream) try {
  ARGCHK(check_nf(nf, TEMXV_NF_MAX) | check_null(src_host, "src_host") | check_null(dst_host, "dst_host") |
         check_null(plev_pa_host, "plev_pa_host") | check_null(ps_or_p, "ps_or_p") | check_dtype(dtype, "dtype") |
         check_dtype(p_dtype, "p_dtype") | check_method_edge(method, edge) | check_sizes(ncol, nlev, nt, "nt", /*remap=*/true, nplev));
  if (pmode != TEMXV_P_HYBRID && pmode != TEMXV_P_FIELD) return fail(TEMX_EINVAL, "pmode must be TEMXV_P_HYBRID or TEMXV_P_FIELD");
  const bool hyb = pmode == TEMXV_P_HYBRID;
  if (hyb && (!hyam_host || !hybm_host)) return fail(TEMX_EINVAL, "hybrid mode needs hyam and hybm");
  if (!hyb) hyam_host = hybm_host = nullptr;   // read in hybrid mode only
  ARGCHK(check_levels(nplev, plev_pa_host, nlev, hyam_host, hybm_host, p0_hybrid));
  int src_dtype[TEMXV_NF_MAX];
  std::fill(src_dtype, src_dtype + nf, dtype);
  const size_t in_elems = (size_t)ncol * nlev * nt;
  ARGCHK(check_fields({nf, src_host, src_dtype, in_elems, dst_host, "dst", dtype, (size_t)ncol * nplev * nt, ps_or_p,
                       "ps_or_p", p_dtype, hyb ? (size_t)ncol * nt : in_elems}));
  int map = 0;   // 0 by row length, 1 lanes along time, 2 slab staged
  if (const char* m = getenv("TEMXV_MAP")) map = !strcmp(m, "time") ? 1 : !strcmp(m, "slab") ? 2 : 0;
  HIPCHK(hipSetDevice(device));
  VertTab tb;
  if (int rc = vert_tab_on(device, nlev, hyam_host, hybm_host, nplev, plev_pa_host, method, &tb)) return rc;
  const int p_f32 = p_dtype == TEMX_F32, logp = method == TEMXV_LOG, hold = edge == TEMXV_EDGE_HOLD;
  hipStream_t st = S_(stream);
#define TEMXV_GO(T, H) \
  launch_vert_nf<T, H>(nf, src_host, dst_host, ncol, nlev, nt, nplev, tb, p0_hybrid, ps_or_p, p_f32, logp, hold, map, st)
  if (dtype == TEMX_F64) return hyb ? TEMXV_GO(double, true) : TEMXV_GO(double, false);
  return hyb ? TEMXV_GO(float, true) : TEMXV_GO(float, false);
#undef TEMXV_GO
} TEMX_CATCH

// ---- time-major records to the engine's layout (include/temx_layout.h) ---------------------------
int temxl_version(void) { return 100; }

int temxl_to_engine(int device, int nf, const void* const* src_host, const int* src_dtype_host, void* const* dst_host,
                    int dst_dtype, int64_t ncol, int nlev, int64_t nt_src, int64_t t0, int64_t ntb, int flags,
                    void* stream) try {
  ARGCHK(check_nf(nf, TEMXL_NF_MAX) | check_null(src_host, "src_host") | check_null(src_dtype_host, "src_dtype_host") |
         check_null(dst_host, "dst_host") | check_dtype(dst_dtype, "dst_dtype") | check_sizes(ncol, nlev, nt_src, "nt_src") |
         check_window(nt_src, t0, ntb) | check_flags(flags, TEMXL_FLIP_LEV));
  ARGCHK(check_fields({nf, src_host, src_dtype_host, (size_t)ncol * nlev * nt_src, dst_host, "dst", dst_dtype,
                       (size_t)ncol * nlev * ntb}));
  const size_t dsz = dtype_size(dst_dtype);
  const unsigned src_f32 = f32_mask(nf, src_dtype_host);
  if (ncol > (int64_t(1) << 35)) return fail(TEMX_EUNSUPPORTED, "too many columns for one launch");
  const LayoutTile tl = layout_tile(ncol, nlev, ntb, dsz);
  const int64_t grid = (int64_t)tl.nct * nf * tl.nlt * tl.ntt;
  if (grid >= (int64_t(1) << 32) / LAYOUT_THREADS)   // HIP takes fewer than 2^32 threads per grid dimension
    return fail(TEMX_EUNSUPPORTED, "too many tiles for one launch (%lld): move the fields or the window in parts", (long long)grid);
  const size_t lds = ((size_t)1 << tl.tc_shift) * tl.stride * dsz;
  if (lds > (size_t)LAYOUT_LDS_BYTES) return fail(TEMX_EINTERNAL, "re-layout tile of %zu bytes exceeds its LDS budget", lds);
  LayoutPtrs fp{};
  for (int f = 0; f < nf; ++f) fp.src[f] = src_host[f], fp.dst[f] = dst_host[f];
  HIPCHK(hipSetDevice(device));
  hipStream_t st = S_(stream);
  const int flip = (flags & TEMXL_FLIP_LEV) ? 1 : 0;
  if (dst_dtype == TEMX_F64)
    hipLaunchKernelGGL((layout_to_engine_kernel<uint64_t>), dim3((unsigned)grid), dim3(LAYOUT_THREADS), lds, st, fp, nf,
                       src_f32, ncol, nlev, t0, ntb, flip, tl);
  else
    hipLaunchKernelGGL((layout_to_engine_kernel<uint32_t>), dim3((unsigned)grid), dim3(LAYOUT_THREADS), lds, st, fp, nf,
                       src_f32, ncol, nlev, t0, ntb, flip, tl);
  HIPCHK(hipGetLastError());
  return TEMX_OK;
} TEMX_CATCH


// ---- time-major model-level records to pressure levels in the engine's layout (include/temx_ingest.h) ----
int temxi_version(void) { return 100; }

int temxi_records_to_pressure(int device, int nf, const void* const* src_host, const int* src_dtype_host,
                              void* const* dst_host, int dst_dtype, int64_t ncol, int nlev, int64_t nt_src, int64_t t0,
                              int64_t ntb, int nplev, const double* plev_pa_host, const double* hyam_host,
                              const double* hybm_host, double p0_hybrid, const void* ps, int ps_dtype, int method,
                              int edge, void* stream) try {
  ARGCHK(check_nf(nf, TEMXI_NF_MAX) | check_null(src_host, "src_host") | check_null(src_dtype_host, "src_dtype_host") |
         check_null(dst_host, "dst_host"));
  if (!plev_pa_host || !hyam_host || !hybm_host) return fail(TEMX_EINVAL, "plev_pa_host, hyam_host or hybm_host is null");
  ARGCHK(check_null(ps, "ps") | check_dtype(dst_dtype, "dst_dtype") | check_dtype(ps_dtype, "ps_dtype") |
         check_method_edge(method, edge) | check_sizes(ncol, nlev, nt_src, "nt_src", /*remap=*/true, nplev) |
         check_window(nt_src, t0, ntb, /*remap=*/true));
  ARGCHK(check_levels(nplev, plev_pa_host, nlev, hyam_host, hybm_host, p0_hybrid));
  ARGCHK(check_fields({nf, src_host, src_dtype_host, (size_t)ncol * nlev * nt_src, dst_host, "dst", dst_dtype,
                       (size_t)ncol * nplev * ntb, ps, "ps", ps_dtype, (size_t)ncol * nt_src}));
  const size_t dsz = dtype_size(dst_dtype);
  const unsigned src_f32 = f32_mask(nf, src_dtype_host);
  const size_t ssz = src_f32 ? 4 : 8;   // the narrowest source
  if (ncol > (int64_t(1) << 34)) return fail(TEMX_EUNSUPPORTED, "too many columns for one launch");
  IngestTile tl{};
  size_t lds = 0;
  if (!ingest_tile(ncol, nlev, ntb, nf, dsz, ssz, &tl, &lds))
    return fail(TEMX_EUNSUPPORTED, "no tile of this shape fits the LDS budget of %d bytes", (int)INGEST_LDS_BYTES);
  const int64_t grid = (int64_t)tl.nct * tl.ntt;
  if (grid >= (int64_t(1) << 32) / INGEST_THREADS)   // HIP takes fewer than 2^32 threads per grid dimension
    return fail(TEMX_EUNSUPPORTED, "too many tiles for one launch (%lld): move the window in parts", (long long)grid);
  if (lds > (size_t)INGEST_LDS_BYTES) return fail(TEMX_EINTERNAL, "ingest tile of %zu bytes exceeds its LDS budget", lds);
  HIPCHK(hipSetDevice(device));
  VertTab tb;   // the tables temxv_interp forms in hybrid mode, through the same cache
  if (int rc = vert_tab_on(device, nlev, hyam_host, hybm_host, nplev, plev_pa_host, method, &tb)) return rc;
  IngestPtrs fp{};
  for (int f = 0; f < nf; ++f) fp.src[f] = src_host[f], fp.dst[f] = dst_host[f];
  const int ps_f32 = ps_dtype == TEMX_F32, logp = method == TEMXV_LOG, hold = edge == TEMXV_EDGE_HOLD;
  hipStream_t st = S_(stream);
#define TEMXI_GO(T, NF)                                                                                              \
  hipLaunchKernelGGL((ingest_kernel<T, NF>), dim3((unsigned)grid), dim3(INGEST_THREADS), lds, st, fp, nf, src_f32, ncol, \
                     nlev, t0, ntb, nplev, tb, p0_hybrid, ps, ps_f32, logp, hold, tl)
  if (dst_dtype == TEMX_F64) {
    if (nf <= 4) TEMXI_GO(double, 4);
    else TEMXI_GO(double, INGEST_NFMAX);
  } else {
    if (nf <= 4) TEMXI_GO(float, 4);
    else TEMXI_GO(float, INGEST_NFMAX);
  }
#undef TEMXI_GO
  HIPCHK(hipGetLastError());
  return TEMX_OK;
} TEMX_CATCH

// ---- time-mean TEM: the sum over time and the epilogue on the caller's zonal means (include/temx_clim.h) ----
int temxc_version(void) { return 100; }

int temxc_time_sum(int device, int nf, const void* const* src_host, const int* src_dtype_host, double* const* acc_host,
                   int64_t ncol, int nlev, int64_t nt, int flags, void* stream) try {
  ARGCHK(check_nf(nf, TEMXC_NF_MAX) | check_null(src_host, "src_host") | check_null(src_dtype_host, "src_dtype_host") |
         check_null(acc_host, "acc_host") | check_sizes(ncol, nlev, nt, "nt") | check_flags(flags, TEMXC_ACCUMULATE));
  const int64_t rows = ncol * nlev;
  ARGCHK(check_fields({nf, src_host, src_dtype_host, (size_t)rows * nt, (void* const*)acc_host, "acc", TEMX_F64, (size_t)rows}));
  // the fp64 and the fp32 sources go in a launch each: their rows are cut differently (clim_shapes.hpp)
  ClimPtrs p64{}, p32{};
  int n64 = 0, n32 = 0;
  for (int f = 0; f < nf; ++f) {
    if (src_dtype_host[f] == TEMX_F64) p64.src[n64] = src_host[f], p64.acc[n64++] = acc_host[f];
    else p32.src[n32] = src_host[f], p32.acc[n32++] = acc_host[f];
  }
  HIPCHK(hipSetDevice(device));
  hipStream_t st = S_(stream);
  const int accumulate = (flags & TEMXC_ACCUMULATE) ? 1 : 0;
  int rc;
  if (n64 && (rc = launch_time_sum<double>(p64, n64, rows, nt, accumulate, st))) return rc;
  if (n32 && (rc = launch_time_sum<float>(p32, n32, rows, nt, accumulate, st))) return rc;
  return TEMX_OK;
} TEMX_CATCH

int temxc_tem_from_zonal_means(temx_plan* pl, double* zm8, int64_t nts, double* results, double* zonal, void* stream) try {
  int rc = tem_ready(pl);
  if (rc) return rc;
  if (!zm8 || !results) return fail(TEMX_EINVAL, "null argument");
  if (nts < 1) return fail(TEMX_EINVAL, "nts must be at least 1");
  if ((double)pl->M * (double)pl->nlev * (double)nts >= 2147483648.0)
    return fail(TEMX_EUNSUPPORTED, "M * nlev * nts = %.0f is too large for one launch", (double)pl->M * pl->nlev * (double)nts);
  HIPCHK(hipSetDevice(pl->device));
  return tem_epilogue_on(pl, zm8, nts, results, zonal, S_(stream));
} TEMX_CATCH

// ---- time-mean TEM in missing-value mode: the sum over the valid times (include/temx_nclim.h, kernels_nclim.hpp) ----
int temxn_version(void) { return 100; }

int temxn_time_sum_valid(int device, int nf, const void* const* src_host, int src_dtype, double* const* acc_host,
                         double* const* cnt_host, int64_t ncol, int nlev, int64_t nt, int flags, void* stream) try {
  ARGCHK(check_nf(nf, TEMXN_NF_MAX) | check_null(src_host, "src_host") | check_null(acc_host, "acc_host") |
         check_null(cnt_host, "cnt_host") | check_dtype(src_dtype, "src_dtype") | check_sizes(ncol, nlev, nt, "nt") |
         check_flags(flags, TEMXN_ACCUMULATE | TEMXN_COMMON_MASK));
  const int64_t rows = ncol * nlev;
  const bool common = (flags & TEMXN_COMMON_MASK) != 0;
  ARGCHK(check_sum_valid(nf, src_host, src_dtype, (size_t)rows * nt, acc_host, cnt_host, common ? 1 : nf, (size_t)rows));
  NclimPtrs fp{};
  for (int f = 0; f < nf; ++f) fp.src[f] = src_host[f], fp.acc[f] = acc_host[f], fp.cnt[f] = cnt_host[common ? 0 : f];
  HIPCHK(hipSetDevice(device));
  const int accumulate = (flags & TEMXN_ACCUMULATE) ? 1 : 0;
  if (src_dtype == TEMX_F64) return launch_time_sum_valid_nf<double>(fp, nf, common, rows, nt, accumulate, S_(stream));
  return launch_time_sum_valid_nf<float>(fp, nf, common, rows, nt, accumulate, S_(stream));
} TEMX_CATCH

// ---- grouped and weighted time means: the segmented sum over time (include/temx_gclim.h, kernels_gclim.hpp) ----
int temxg_version(void) { return 100; }

int temxg_time_sum_groups(int device, int nf, const void* const* src_host, const int* src_dtype_host, double* const* acc_host,
                          int64_t ncol, int nlev, int64_t nt, int64_t nt_record, int64_t t0, int ng,
                          const int32_t* label_host, const double* weight_host_or_null, int flags, void* stream) try {
  ARGCHK(check_nf(nf, TEMXG_NF_MAX) | check_null(src_host, "src_host") | check_null(src_dtype_host, "src_dtype_host") |
         check_null(acc_host, "acc_host") | check_sizes(ncol, nlev, nt, "nt") | check_flags(flags, TEMXG_ACCUMULATE));
  ARGCHK(check_groups(ng, TEMXG_NG_MAX, nt_record, t0, nt, label_host, weight_host_or_null));
  const int64_t rows = ncol * nlev;
  ARGCHK(check_fields({nf, src_host, src_dtype_host, (size_t)rows * nt, (void* const*)acc_host, "acc", TEMX_F64, (size_t)rows * ng}));
  // the fp64 and the fp32 sources go in a launch each: their rows are cut differently (clim_shapes.hpp)
  ClimPtrs p64{}, p32{};
  int n64 = 0, n32 = 0;
  for (int f = 0; f < nf; ++f) {
    if (src_dtype_host[f] == TEMX_F64) p64.src[n64] = src_host[f], p64.acc[n64++] = acc_host[f];
    else p32.src[n32] = src_host[f], p32.acc[n32++] = acc_host[f];
  }
  HIPCHK(hipSetDevice(device));
  hipStream_t st = S_(stream);
  const int accumulate = (flags & TEMXG_ACCUMULATE) ? 1 : 0;
  GclimTab tb{};
  GclimWindow win{};
  int rc = gclim_tables(device, ng, nt_record, label_host, weight_host_or_null, &tb, &win, t0, nt);
  if (rc) return rc;
  if (win.np == 0) {   // no labelled time in the block: nothing to add, or all zeros
    for (int f = 0; f < nf && !accumulate; ++f) HIPCHK(hipMemsetAsync(acc_host[f], 0, (size_t)rows * ng * sizeof(double), st));
    return TEMX_OK;
  }
  if (n64 && (rc = launch_time_sum_groups<double>(p64, n64, rows, nt, t0, tb, win, accumulate, st))) return rc;
  if (n32 && (rc = launch_time_sum_groups<float>(p32, n32, rows, nt, t0, tb, win, accumulate, st))) return rc;
  return TEMX_OK;
} TEMX_CATCH

// ---- masked grouped time means: the grouped sum over the valid times (../include/temx_mgclim.h, kernels_mgclim.hpp) ----
int temxw_version(void) { return 100; }

int temxw_time_sum_groups_valid(int device, int nf, const void* const* src_host, int src_dtype, double* const* acc_host,
                                double* const* wsum_host, double* const* cnt_host, int64_t ncol, int nlev, int64_t nt,
                                int64_t nt_record, int64_t t0, int ng, const int32_t* label_host,
                                const double* weight_host_or_null, int flags, void* stream) try {
  ARGCHK(check_nf(nf, TEMXW_NF_MAX) | check_null(src_host, "src_host") | check_null(acc_host, "acc_host") |
         check_null(wsum_host, "wsum_host") | check_null(cnt_host, "cnt_host") | check_dtype(src_dtype, "src_dtype") |
         check_sizes(ncol, nlev, nt, "nt") | check_flags(flags, TEMXW_ACCUMULATE | TEMXW_COMMON_MASK));
  ARGCHK(check_groups(ng, TEMXW_NG_MAX, nt_record, t0, nt, label_host, weight_host_or_null));
  const int64_t rows = ncol * nlev;
  const bool common = (flags & TEMXW_COMMON_MASK) != 0;
  const int nextra = common ? 1 : nf;
  ARGCHK(check_sum_groups_valid(nf, src_host, src_dtype, (size_t)rows * nt, acc_host, wsum_host, cnt_host, nextra,
                                (size_t)rows * ng));
  MgclimPtrs fp{};
  for (int f = 0; f < nf; ++f)
    fp.src[f] = src_host[f], fp.acc[f] = acc_host[f], fp.wsum[f] = wsum_host[common ? 0 : f], fp.cnt[f] = cnt_host[common ? 0 : f];
  HIPCHK(hipSetDevice(device));
  hipStream_t st = S_(stream);
  const int accumulate = (flags & TEMXW_ACCUMULATE) ? 1 : 0;
  GclimTab tb{};
  GclimWindow win{};
  int rc = gclim_tables(device, ng, nt_record, label_host, weight_host_or_null, &tb, &win, t0, nt);
  if (rc) return rc;
  if (win.np == 0) {   // no labelled time in the block: nothing to add, or all zeros
    const size_t bytes = (size_t)rows * ng * sizeof(double);
    for (int f = 0; f < nf && !accumulate; ++f) {
      HIPCHK(hipMemsetAsync(acc_host[f], 0, bytes, st));
      if (f < nextra) {
        HIPCHK(hipMemsetAsync(wsum_host[f], 0, bytes, st));
        HIPCHK(hipMemsetAsync(cnt_host[f], 0, bytes, st));
      }
    }
    return TEMX_OK;
  }
  if (src_dtype == TEMX_F64)
    return launch_time_sum_groups_valid_nf<double>(device, fp, nf, common, rows, nt, t0, tb, win, accumulate, st);
  return launch_time_sum_groups_valid_nf<float>(device, fp, nf, common, rows, nt, t0, tb, win, accumulate, st);
} TEMX_CATCH

// ---- tracer TEM in missing-value mode (include/temx_mtracer.h, kernels_mtracer.hpp) ----
int temxm_version(void) { return 100; }

// everything the two calls refuse, before any device call
static int mtracer_ready(temx_plan* pl, const void* q, const void* va, const void* wap, const void* out, int dtype) {
  if (!pl || !q || !va || !wap || !out) return fail(TEMX_EINVAL, "null argument");
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  if (!miss_mode(pl))
    return fail(TEMX_ESTATE, "the plan is not in missing-value mode (TEMX_OPT_MISSING = 1): temx_tracer_run serves it");
  if (int rc = tem_ready(pl)) return rc;
  if (!pl->miss_valid)
    return fail(TEMX_ESTATE, "missing-value mode: the tracer needs a masked temx_tem_run on this plan first");
  return TEMX_OK;
}

int temxm_tracer_run(temx_plan* pl, const void* q, const void* va, const void* wap, int dtype, double* tres,
                     double* tzon, double* tcov, void* stream) try {
  int rc = mtracer_ready(pl, q, va, wap, tres, dtype);
  if (rc) return rc;
  HIPCHK(hipSetDevice(pl->device));
  const int64_t D = pl->D, KD = (int64_t)pl->K * D, MD = (int64_t)pl->M * D;
  const size_t slab = (size_t)pl->K4 * D * 8;
  if ((rc = pl->mtB.ensure((size_t)(KD + (int64_t)pl->NE * D) * 8))) return rc;
  if ((rc = pl->mtB2.ensure((size_t)2 * KD * 8))) return rc;
  if ((rc = pl->mtC.ensure(3 * slab))) return rc;
  if ((rc = pl->mtCcov.ensure(slab))) return rc;
  if ((rc = pl->mtz.ensure((size_t)3 * MD * 8))) return rc;
  hipStream_t st = S_(stream);
  pl->mt_valid = false;
  FieldPtrs<3> f3;
  f3.p[0] = q; f3.p[1] = va; f3.p[2] = wap;
  const double* E = pl->mtB.d() + KD;
  TimedLaunch tl{};
  time_begin(pl, 0, st, tl);
  rc = launch_miss_tracer_project(pl, f3, dtype, pl->mtB.d(), st);
  time_end(pl, 0, st, tl);
  if (rc) return rc;
  // Ct = (C_q, C_v, C_omega): C_q and the tracer's coverage coefficients from its own systems, qb -> tz[0]; v and
  // omega keep the masked coefficients of the TEM run
  if ((rc = launch_miss_system<1>(pl, pl->mtB.d(), E, D, pl->mtC.d(), pl->mtCcov.d(), pl->mtz.d(), tcov, st))) return rc;
  HIPCHK(hipMemcpyAsync((char*)pl->mtC.p + slab, (char*)pl->mC.p + slab, slab, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync((char*)pl->mtC.p + 2 * slab, (char*)pl->mC.p + 3 * slab, slab, hipMemcpyDeviceToDevice, st));
  TimedLaunch tl2{};
  time_begin(pl, 1, st, tl2);
  rc = launch_miss_tracer_eddy(pl, four(q, va, wap, nullptr), dtype, st);
  time_end(pl, 1, st, tl2);
  if (rc) return rc;
  const int slabs = pl->sp_eddy.nsplit * (8 / pl->sp_eddy.dpw);
  if ((rc = launch_reduce(pl, pl->partial.d(), slabs, 2 * KD, pl->mtB2.d(), st))) return rc;
  // qpvpb qpwappb -> tz[1..2] with the tracer's systems
  if ((rc = launch_miss_system<2>(pl, pl->mtB2.d(), E, D, nullptr, nullptr, pl->mtz.d() + MD, nullptr, st))) return rc;
  EpiTables tb{pl->p.d(), pl->pg.d(), pl->lg.d(), pl->coslat.d(), pl->fcor.d()};
  hipLaunchKernelGGL(tracer_epilogue_kernel, dim3((unsigned)((MD + 255) / 256)), dim3(256), 0, st, pl->zb.d(),
                     pl->mtz.d(), pl->M, pl->nlev, pl->nt, tb, pl->p0, tres, tzon);
  HIPCHK(hipGetLastError());
  pl->mt_valid = true;
  return TEMX_OK;
} TEMX_CATCH

int temxm_tracer_eddy(temx_plan* pl, const void* q, const void* va, const void* wap, int dtype,
                      double* const* ptrs3_host, void* stream) try {
  int rc = mtracer_ready(pl, q, va, wap, ptrs3_host, dtype);
  if (rc) return rc;
  if (!pl->mt_valid)
    return fail(TEMX_ESTATE, "missing-value mode: no temxm_tracer_run since the latest masked temx_tem_run on this plan");
  HIPCHK(hipSetDevice(pl->device));
  FieldPtrs<3> f3;
  f3.p[0] = q; f3.p[1] = va; f3.p[2] = wap;
  TracerEddyOut eo{{ptrs3_host[0], ptrs3_host[1], ptrs3_host[2]}};
  return launch_miss_tracer_native(pl, f3, dtype, eo, S_(stream));
} TEMX_CATCH

// ---- zonal wavenumbers: wave-m components and eddy fluxes (../include/temx_wave.h, kernels_wave.hpp) ----
int temxk_version(void) { return 100; }

int temxk_wave_create(temxk_wave** out, temx_plan* pl, const double* lon_deg_host, int nm, const int* m_host) try {
  if (!out) return fail(TEMX_EINVAL, "null argument");
  *out = nullptr;
  if (!pl) return fail(TEMX_EINVAL, "null plan");
  if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
  char msg[256];
  if (const int code = wave_check_args(pl->L, pl->N, lon_deg_host, nm, m_host, msg, sizeof msg)) return fail(code, "%s", msg);
  if (int rc = wave_plan_refused(pl)) return rc;
  HIPCHK(hipSetDevice(pl->device));
  HIPCHK(hipDeviceSynchronize());
  temxk_wave* w = new temxk_wave();
  w->pl = pl;
  w->device = pl->device;
  auto bail = [&](int code) {
    delete w;
    return code;
  };
  const double d2r = M_PI / 180.0;
  std::vector<double> lat((size_t)pl->N), lon((size_t)pl->N), lat_out((size_t)pl->M);
  for (int64_t i = 0; i < pl->N; ++i) lat[(size_t)i] = pl->h_lat[(size_t)i] * d2r, lon[(size_t)i] = lon_deg_host[i] * d2r;
  for (int j = 0; j < pl->M; ++j) lat_out[(size_t)j] = pl->lat_out_deg[(size_t)j] * d2r;
  int rc, zero = 0;
  if ((rc = upload(w->lat, lat)) || (rc = upload(w->lon, lon)) || (rc = upload(w->lat_out, lat_out)) ||
      (rc = upload(w->flag, &zero, sizeof zero)))
    return bail(rc);
  w->ms.resize((size_t)nm);
  for (int i = 0; i < nm; ++i) {
    w->ms[(size_t)i].m = m_host[i];
    w->ms[(size_t)i].sh = wave_shape(pl->L, m_host[i]);
    w->kc_max = std::max(w->kc_max, w->ms[(size_t)i].sh.Kc);
  }
  for (WaveM& wm : w->ms)
    if ((rc = wave_build_m(w, wm))) return bail(rc);
  *out = w;
  return TEMX_OK;
} TEMX_CATCH

void temxk_wave_destroy(temxk_wave* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);   // (the plan may be gone already)
  (void)hipDeviceSynchronize();
  delete w;
}

int64_t temxk_wave_workspace_bytes(const temxk_wave* w) {
  if (!w) return 0;
  size_t n = w->lat.bytes + w->lon.bytes + w->lat_out.bytes + w->partial.bytes + w->B.bytes + w->C.bytes + w->flag.bytes;
  for (const WaveM& wm : w->ms) n += wm.yblk.bytes + wm.pz.bytes + wm.ginv.bytes;
  return (int64_t)n;
}

int temxk_wave_project(temxk_wave* w, int mi, int nf, const void* const* fields_host, const int* dtype_host, int64_t D,
                       double* parts, double* coef_or_null, void* stream) try {
  if (!w || !fields_host || !dtype_host || !parts) return fail(TEMX_EINVAL, "null argument");
  if (mi < 0 || mi >= (int)w->ms.size()) return fail(TEMX_EINVAL, "mi must lie in 0..%d, got %d", (int)w->ms.size() - 1, mi);
  if (nf < 1 || nf > WAVE_NF_MAX) return fail(TEMX_EINVAL, "nf must lie in 1..%d, got %d", WAVE_NF_MAX, nf);
  for (int f = 0; f < nf; ++f) {
    if (!fields_host[f]) return fail(TEMX_EINVAL, "field %d is null", f);
    if (dtype_host[f] != TEMX_F64 && dtype_host[f] != TEMX_F32) return bad_dtype();
  }
  if (D < 1 || D >= ((int64_t)1 << 28)) return fail(TEMX_EINVAL, "D must be in [1, 2^28)");
  temx_plan* pl = w->pl;
  if (int rc = wave_plan_refused(pl)) return rc;
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  const WaveM& wm = w->ms[(size_t)mi];
  const int64_t KD = (int64_t)wm.sh.Kc * D, MD = (int64_t)pl->M * D;
  int rc;
  if ((rc = wave_ensure(w, 1, D))) return rc;
  for (int f = 0; f < nf; ++f) {
    FieldPtrs<1> fp;
    fp.p[0] = fields_host[f];
    double* C = coef_or_null ? coef_or_null + f * KD : w->C.d();
    if ((rc = wave_sweep<1>(w, wm, fp, dtype_host[f], D, nullptr, -1, w->B.d(), st))) return rc;
    if ((rc = wave_solve(wm, 1, D, w->B.d(), C, st))) return rc;
    hipLaunchKernelGGL(wave_parts_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)pl->M, 1), dim3(256), 0, st,
                       (const double*)C, wm.sh.ndeg, pl->M, D, (const double*)wm.pz.d(), parts + f * 2 * MD);
    HIPCHK(hipGetLastError());
  }
  return TEMX_OK;
} TEMX_CATCH

int temxk_wave_fluxes(temxk_wave* w, const void* ua, const void* va, const void* ta, const void* wap, int dtype,
                      double* flux, double* parts_or_null, void* stream) try {
  if (!w || !ua || !va || !ta || !wap || !flux) return fail(TEMX_EINVAL, "null argument");
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  temx_plan* pl = w->pl;
  if (int rc = tem_ready(pl)) return rc;
  if (int rc = wave_plan_refused(pl)) return rc;
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  const int64_t D = pl->D, MD = (int64_t)pl->M * D;
  int rc;
  if ((rc = wave_ensure(w, 4, D))) return rc;
  const FieldPtrs<4> fp = four(ua, va, ta, wap);
  for (size_t i = 0; i < w->ms.size(); ++i) {
    const WaveM& wm = w->ms[i];
    // theta = T (p0/p)^kappa fused into the load of field 2, as in temx_tem_stage1
    TimedLaunch tl{nullptr, nullptr};
    bool timed = false;
    if (w->timing && w->timed.size() < kMaxTimedLaunches) {
      timed = hipEventCreate(&tl.a) == hipSuccess;
      if (timed && hipEventCreate(&tl.b) != hipSuccess) {
        (void)hipEventDestroy(tl.a);
        timed = false;
      }
      if (timed) (void)hipEventRecord(tl.a, st);
    }
    rc = wave_sweep<4>(w, wm, fp, dtype, D, pl->colscale.d(), 2, w->B.d(), st);
    if (timed) {
      (void)hipEventRecord(tl.b, st);
      w->timed.push_back(tl);
    }
    if (rc) return rc;
    if ((rc = wave_solve(wm, 4, D, w->B.d(), w->C.d(), st))) return rc;
    hipLaunchKernelGGL(wave_flux_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)pl->M), dim3(256), 0, st,
                       (const double*)w->C.d(), wm.sh.ndeg, pl->M, D, (const double*)wm.pz.d(), flux + (int64_t)i * 3 * MD,
                       parts_or_null ? parts_or_null + (int64_t)i * 8 * MD : (double*)nullptr);
    HIPCHK(hipGetLastError());
  }
  return TEMX_OK;
} TEMX_CATCH

// Synchronises the stream and reports whether a non-finite value reached the sums of temxk_wave_project / temxk_wave_fluxes
// since the last call (as temx_status does for the plan's own sums; the two flags are separate).
int temxk_wave_status(temxk_wave* w, int* nonfinite, void* stream) try {
  if (!w || !nonfinite) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(w->device));
  HIPCHK(hipStreamSynchronize(S_(stream)));
  int f = 0, zero = 0;
  HIPCHK(hipMemcpy(&f, w->flag.p, sizeof f, hipMemcpyDeviceToHost));
  if (f) HIPCHK(hipMemcpy(w->flag.p, &zero, sizeof zero, hipMemcpyHostToDevice));
  *nonfinite = f != 0;
  return TEMX_OK;
} TEMX_CATCH

// wave_shape of wave_tables.hpp, for callers that size buffers or report the stored bytes (no device, no state)
int temxk_wave_shape(int L, int m, int* shape6_host) try {
  if (!shape6_host) return fail(TEMX_EINVAL, "null argument");
  if (L < 1 || L > 511 || m < 1 || m > L) return fail(TEMX_EINVAL, "L must lie in 1..511 and m in 1..L, got L = %d, m = %d", L, m);
  const WaveShape s = wave_shape(L, m);
  const int v[6] = {s.ndeg, s.Kc, s.nslice, s.tb_last, s.gstride, s.kpad};
  std::copy(v, v + 6, shape6_host);
  return TEMX_OK;
} TEMX_CATCH

// measurement helper (tools/wave_bench.py; not on the product path): events around the projection sweeps (sweep and slab
// reduction) of temxk_wave_fluxes.  Enabling or disabling drops the events recorded so far.
int temxk_wave_timing(temxk_wave* w, int enable) try {
  if (!w) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(w->device));
  w->drop_events();
  w->timing = enable != 0;
  return TEMX_OK;
} TEMX_CATCH

int temxk_wave_timing_read(temxk_wave* w, double* sum_ms, int* launches) try {
  if (!w || !sum_ms || !launches) return fail(TEMX_EINVAL, "null argument");
  HIPCHK(hipSetDevice(w->device));
  double tot = 0.0;
  for (auto& tl : w->timed) {
    HIPCHK(hipEventSynchronize(tl.b));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, tl.a, tl.b));
    tot += ms;
  }
  *sum_ms = tot;
  *launches = (int)w->timed.size();
  return TEMX_OK;
} TEMX_CATCH

// ---- zonal wavenumbers on latitude classes (../include_wavecls/temx_wavecls.h, kernels_wavecls.hpp, wave_class_tables.hpp) ----
int temxz_version(void) { return 100; }

int temxz_wave_create(temxz_wave** out, temx_plan* pl, const double* lon_deg_host, int nm, const int* m_host) try {
  if (!out) return fail(TEMX_EINVAL, "null argument");
  *out = nullptr;
  if (!pl) return fail(TEMX_EINVAL, "null plan");
  if (!pl->finalized) return fail(TEMX_ESTATE, "plan not finalised");
  char msg[256];
  if (const int code = wave_check_args(pl->L, pl->N, lon_deg_host, nm, m_host, msg, sizeof msg)) return fail(code, "%s", msg);
  if (int rc = wavecls_plan_refused(pl)) return rc;
  for (int i = 0; i < nm; ++i)
    if (wave_ndeg(pl->L, m_host[i]) > WAVECLS_NDEG_MAX)
      return fail(TEMX_EUNSUPPORTED, "wavenumber %d at L = %d has %d degrees: the class form serves at most %d; use the generic form",
                  m_host[i], pl->L, wave_ndeg(pl->L, m_host[i]), WAVECLS_NDEG_MAX);
  HIPCHK(hipSetDevice(pl->device));
  HIPCHK(hipDeviceSynchronize());
  temxz_wave* z = new temxz_wave();
  temxk_wave* w = &z->g;
  w->pl = pl;
  w->device = pl->device;
  auto bail = [&](int code) {
    delete z;
    return code;
  };
  const double d2r = M_PI / 180.0;
  std::vector<double> lat((size_t)pl->N), lon((size_t)pl->N), lat_out((size_t)pl->M);
  for (int64_t i = 0; i < pl->N; ++i) lat[(size_t)i] = pl->h_lat[(size_t)i] * d2r, lon[(size_t)i] = lon_deg_host[i] * d2r;
  for (int j = 0; j < pl->M; ++j) lat_out[(size_t)j] = pl->lat_out_deg[(size_t)j] * d2r;
  int rc, zero = 0;
  DevBuf rep;                   // one representative row per class and side: build time only
  struct Free {
    DevBuf& a;
    ~Free() { a.release(); }
  } free_{rep};
  if ((rc = upload(w->lat, lat)) || (rc = upload(w->lon, lon)) || (rc = upload(w->lat_out, lat_out)) ||
      (rc = upload(w->flag, &zero, sizeof zero)) ||
      (rc = upload(rep, wavecls_representatives(pl->h_crow, pl->gbatch0, pl->cgroups))))
    return bail(rc);
  w->ms.resize((size_t)nm);
  z->cm.resize((size_t)nm);
  for (int i = 0; i < nm; ++i) {
    w->ms[(size_t)i].m = m_host[i];
    w->ms[(size_t)i].sh = wave_shape(pl->L, m_host[i]);
    z->cm[(size_t)i].sh = wavecls_shape(pl->L, m_host[i]);
    w->kc_max = std::max(w->kc_max, w->ms[(size_t)i].sh.Kc);
  }
  for (int i = 0; i < nm; ++i) {
    WaveClsM& cm = z->cm[(size_t)i];
    if ((rc = upload(cm.cw, wavecls_weights(pl->h_crow, lon.data(), m_host[i])))) return bail(rc);
    if ((rc = wave_build_m(w, w->ms[(size_t)i], &cm, static_cast<const int*>(rep.p)))) return bail(rc);
  }
  w->partial.release();          // the slabs of the Gram sweeps: sized for the generic sweep
  *out = z;
  return TEMX_OK;
} TEMX_CATCH

void temxz_wave_destroy(temxz_wave* z) {
  if (!z) return;
  (void)hipSetDevice(z->g.device);   // (the plan may be gone already)
  (void)hipDeviceSynchronize();
  delete z;
}

int64_t temxz_wave_workspace_bytes(const temxz_wave* z) {
  if (!z) return 0;
  size_t n = (size_t)temxk_wave_workspace_bytes(&z->g);
  for (const WaveClsM& c : z->cm) n += c.tab.bytes + c.cw.bytes;
  return (int64_t)n;
}

int temxz_wave_project(temxz_wave* z, int mi, int nf, const void* const* fields_host, const int* dtype_host, int64_t D,
                       double* parts, double* coef_or_null, void* stream) try {
  if (!z || !fields_host || !dtype_host || !parts) return fail(TEMX_EINVAL, "null argument");
  temxk_wave* w = &z->g;
  if (mi < 0 || mi >= (int)w->ms.size()) return fail(TEMX_EINVAL, "mi must lie in 0..%d, got %d", (int)w->ms.size() - 1, mi);
  if (nf < 1 || nf > WAVE_NF_MAX) return fail(TEMX_EINVAL, "nf must lie in 1..%d, got %d", WAVE_NF_MAX, nf);
  for (int f = 0; f < nf; ++f) {
    if (!fields_host[f]) return fail(TEMX_EINVAL, "field %d is null", f);
    if (dtype_host[f] != TEMX_F64 && dtype_host[f] != TEMX_F32) return bad_dtype();
  }
  if (D < 1 || D >= ((int64_t)1 << 28)) return fail(TEMX_EINVAL, "D must be in [1, 2^28)");
  temx_plan* pl = w->pl;
  if (int rc = wavecls_plan_refused(pl)) return rc;
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  const WaveM& wm = w->ms[(size_t)mi];
  const int64_t KD = (int64_t)wm.sh.Kc * D, MD = (int64_t)pl->M * D;
  int rc;
  if ((rc = wave_ensure(w, 1, D))) return rc;
  for (int f = 0; f < nf; ++f) {
    FieldPtrs<1> fp;
    fp.p[0] = fields_host[f];
    double* C = coef_or_null ? coef_or_null + f * KD : w->C.d();
    if ((rc = wavecls_sweep<1>(z, (size_t)mi, fp, dtype_host[f], D, nullptr, -1, w->B.d(), st))) return rc;
    if ((rc = wave_solve(wm, 1, D, w->B.d(), C, st))) return rc;
    hipLaunchKernelGGL(wave_parts_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)pl->M, 1), dim3(256), 0, st,
                       (const double*)C, wm.sh.ndeg, pl->M, D, (const double*)wm.pz.d(), parts + f * 2 * MD);
    HIPCHK(hipGetLastError());
  }
  return TEMX_OK;
} TEMX_CATCH

int temxz_wave_fluxes(temxz_wave* z, const void* ua, const void* va, const void* ta, const void* wap, int dtype,
                      double* flux, double* parts_or_null, void* stream) try {
  if (!z || !ua || !va || !ta || !wap || !flux) return fail(TEMX_EINVAL, "null argument");
  if (dtype != TEMX_F64 && dtype != TEMX_F32) return bad_dtype();
  temxk_wave* w = &z->g;
  temx_plan* pl = w->pl;
  if (int rc = tem_ready(pl)) return rc;
  if (int rc = wavecls_plan_refused(pl)) return rc;
  HIPCHK(hipSetDevice(pl->device));
  hipStream_t st = S_(stream);
  const int64_t D = pl->D, MD = (int64_t)pl->M * D;
  int rc;
  if ((rc = wave_ensure(w, 4, D))) return rc;
  const FieldPtrs<4> fp = four(ua, va, ta, wap);
  for (size_t i = 0; i < w->ms.size(); ++i) {
    const WaveM& wm = w->ms[i];
    // theta = T (p0/p)^kappa: the column scale of field 2, applied to its class sums (the sweep is linear)
    if ((rc = wavecls_sweep<4>(z, i, fp, dtype, D, pl->colscale.d(), 2, w->B.d(), st))) return rc;
    if ((rc = wave_solve(wm, 4, D, w->B.d(), w->C.d(), st))) return rc;
    hipLaunchKernelGGL(wave_flux_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)pl->M), dim3(256), 0, st,
                       (const double*)w->C.d(), wm.sh.ndeg, pl->M, D, (const double*)wm.pz.d(), flux + (int64_t)i * 3 * MD,
                       parts_or_null ? parts_or_null + (int64_t)i * 8 * MD : (double*)nullptr);
    HIPCHK(hipGetLastError());
  }
  return TEMX_OK;
} TEMX_CATCH

int temxz_wave_status(temxz_wave* z, int* nonfinite_host, void* stream) try {
  if (!z || !nonfinite_host) return fail(TEMX_EINVAL, "null argument");
  return temxk_wave_status(&z->g, nonfinite_host, stream);
} TEMX_CATCH

// wavecls_shape of wave_class_tables.hpp (no device, no state)
int temxz_wave_shape(int L, int m, int* shape_host) try {
  if (!shape_host) return fail(TEMX_EINVAL, "null argument");
  if (L < 1 || L > 511 || m < 1 || m > L) return fail(TEMX_EINVAL, "L must lie in 1..511 and m in 1..L, got L = %d, m = %d", L, m);
  if (wave_ndeg(L, m) > WAVECLS_NDEG_MAX)
    return fail(TEMX_EUNSUPPORTED, "L = %d, m = %d has %d degrees: the class form serves at most %d", L, m, wave_ndeg(L, m),
                WAVECLS_NDEG_MAX);
  const WaveClsShape s = wavecls_shape(L, m);
  const int v[5] = {s.ndeg, s.Kc, s.TBS, s.nacc, s.fpw};
  std::copy(v, v + 5, shape_host);
  return TEMX_OK;
} TEMX_CATCH

// the cut of a sweep, as wavecls_sweep makes it (host arithmetic only)
int temxz_wave_launch(const temxz_wave* z, int mi, int nf, int64_t D, int* out_host) try {
  if (!z || !out_host) return fail(TEMX_EINVAL, "null argument");
  if (mi < 0 || mi >= (int)z->cm.size()) return fail(TEMX_EINVAL, "mi must lie in 0..%d, got %d", (int)z->cm.size() - 1, mi);
  if (nf != 1 && nf != 4) return fail(TEMX_EINVAL, "nf must be 1 (the sweep of a projection) or 4 (the sweep of the fluxes), got %d", nf);
  if (D < 1 || D >= ((int64_t)1 << 28)) return fail(TEMX_EINVAL, "D must be in [1, 2^28)");
  const temx_plan* pl = z->g.pl;
  const Split sp = nf == 4 ? wavecls_split<4>(pl, D) : wavecls_split<1>(pl, D);
  out_host[0] = z->cm[(size_t)mi].sh.TBS;
  out_host[1] = sp.ndt;
  out_host[2] = sp.nsplit;
  out_host[3] = wavecls_cuts_inside(pl->gbatch0, pl->cgroups, pl->cbatches, sp.nsplit);
  return TEMX_OK;
} TEMX_CATCH

// ---- EP flux by time scale: the filter along the time axis (../include/temx_tfilt.h, kernels_tfilt.hpp) ----
int temxf_version(void) { return 100; }

int temxf_filter_time(int device, int nf, const void* const* src_host, const int* src_dtype_host, int nb, void* const* dst_host,
                      int dst_dtype, int64_t ncol, int nlev, int64_t nt, int nw, const double* weights, int flags,
                      void* stream) try {
  ARGCHK(tfilt_check_args(nf, src_host, src_dtype_host, nb, dst_host, dst_dtype, ncol, nlev, nt, nw, weights, flags));
  const int64_t rows = ncol * nlev;
  // the fp64 and the fp32 sources go in a launch each: their rows are cut differently (tfilt_shapes.hpp)
  TfiltPtrs p64{}, p32{};
  int n64 = 0, n32 = 0;
  for (int f = 0; f < nf; ++f) {
    TfiltPtrs& p = src_dtype_host[f] == TEMX_F64 ? p64 : p32;
    int& n = src_dtype_host[f] == TEMX_F64 ? n64 : n32;
    p.src[n] = src_host[f];
    for (int b = 0; b < nb; ++b) p.dst[b][n] = dst_host[b * nf + f];
    ++n;
  }
  for (const size_t esz : {sizeof(double), sizeof(float)})   // every refusal before the first launch
    if ((esz == 8 ? n64 : n32) && tfilt_shape(rows, nt, nw, nb, esz, dtype_size(dst_dtype)).grid >= TFILT_GRID_MAX)
      return fail(TEMX_EUNSUPPORTED, "too many rows for one launch: filter the fields in parts along ncol");
  HIPCHK(hipSetDevice(device));
  hipStream_t st = S_(stream);
  int rc;
  if (n64 && (rc = launch_tfilt<double, double>(p64, n64, nb, weights, rows, nt, nw, st))) return rc;
  if (n32 && dst_dtype == TEMX_F64 && (rc = launch_tfilt<float, double>(p32, n32, nb, weights, rows, nt, nw, st))) return rc;
  if (n32 && dst_dtype == TEMX_F32 && (rc = launch_tfilt<float, float>(p32, n32, nb, weights, rows, nt, nw, st))) return rc;
  return TEMX_OK;
} TEMX_CATCH

// tfilt_shape of tfilt_shapes.hpp, for callers that want the edges of the cut (no device, no state)
int temxf_filter_shape(int64_t rows, int64_t nt, int nw, int nb, int src_esz, int dst_esz, int* shape_host) try {
  ARGCHK(check_null(shape_host, "shape_host") | tfilt_check_sizes(rows, 1, nt, nw, nb));
  if ((src_esz != 4 && src_esz != 8) || (dst_esz != 4 && dst_esz != 8)) return fail(TEMX_EINVAL, "src_esz and dst_esz must be 4 or 8");
  if (src_esz == 8 && dst_esz == 4) return fail(TEMX_EINVAL, "src_esz is 8 but dst_esz is 4: an fp64 source has no fp32 destination");
  const TfiltShape s = tfilt_shape(rows, nt, nw, nb, (size_t)src_esz, (size_t)dst_esz);
  if (s.grid >= TFILT_GRID_MAX)
    return fail(TEMX_EUNSUPPORTED, "too many rows for one launch (%lld workgroups): filter the fields in parts along ncol",
                (long long)s.grid);
  const int v[7] = {s.rpb, s.TT, s.stride, s.R, s.ntile, (int)s.grid, (int)tfilt_lds_bytes(s, (size_t)src_esz)};
  std::copy(v, v + 7, shape_host);
  return TEMX_OK;
} TEMX_CATCH

}  // extern "C"
