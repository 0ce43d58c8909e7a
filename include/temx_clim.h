/* temx_clim.h -- fifth header of libtemx.so: the two device steps of a time-mean (climatological) TEM.
 *
 * The time-mean TEM state, the time-mean EP flux and its split into stationary and transient waves need two things
 * the engine of temx.h does not expose: the sum over time of fields in the engine's layout ([ncol][nlev][nt], time
 * fastest), and the epilogue of a TEM run -- the step from the seven zonal means to the ten results -- on zonal means
 * the caller supplies.  Both have a header, a prefix (temxc_) and a version of their own; the entry points of temx.h,
 * temx_vert.h, temx_layout.h and temx_ingest.h and their versions are untouched.
 *
 * Conventions are those of temx.h: device pointers unless the name ends in _host, dtype TEMX_F64 / TEMX_F32, stream a
 * hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h with the message in
 * temx_last_error().  Argument checks come before any device call.  Both calls are asynchronous and stream ordered and
 * allocate nothing.
 *
 * Contract of temxc_time_sum, per field f, column i, level k:
 *   acc[f][i][k] = sum over t of (double) src[f][i][k][t]            (acc[f][i][k] += ... under TEMXC_ACCUMULATE, one
 *   further rounding).  fp32 widens exactly, every addition is fp64.  The sum of a row is a fixed function of its nt
 *   values, nt and the source dtype: it does not depend on ncol, nlev, the row's position, the alignment of the
 *   pointers or the shape of the launch, so equal rows give equal bits and repeated calls are bitwise identical; a row
 *   of one element is that element.  Non-finite values propagate into their own row and no other.  No atomics.  Nothing
 *   is written outside acc[f][0 .. ncol * nlev).
 *
 * Contract of temxc_tem_from_zonal_means: the epilogue of temx_tem_run (int_vbdp, the derivatives, psi and the ten
 *   results, with the same kernels chosen the same way) applied to zm8[0 .. 6], the seven zonal means in TEMX_Z_* order
 *   (ub vb thetab wapb upvpb upwappb vptpb), each [M][nlev][nts]; zm8[7] is scratch the call overwrites (int_vbdp).
 *   It reads the level and latitude tables of the plan only, so nts is any value >= 1 whatever nt the plan was set for,
 *   and it changes no plan state: coefficients, zonal means, stage flags and every later call behave as if it had not
 *   been made.  Allowed on plans in missing-value mode and in the latitude-bin form; NaN in, NaN out by IEEE
 *   propagation.
 */
#ifndef TEMX_CLIM_H
#define TEMX_CLIM_H

#include <stdint.h>

#include "temx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TEMXC_NF_MAX = 8 };
enum { TEMXC_ACCUMULATE = 1 };

int temxc_version(void); /* 100 */

/* nf in 1..TEMXC_NF_MAX fields in one call.  TEMX_EINVAL: nf out of range, a null pointer, an unknown dtype or flag,
 * sizes below 1, a pointer not aligned to its element size, an acc that overlaps a src or another acc.  device is
 * used as given.  TEMX_EUNSUPPORTED: a field needs 2^24 workgroups or more in one launch -- rows of 256 elements or
 * more (512 for fp32) take one wave each, four to a workgroup, so the limit there is ncol * nlev >= 2^26 rows; shorter
 * rows go at least 16 to a workgroup.  Sum such fields in parts along ncol. */
int temxc_time_sum(int device, int nf,
                   const void* const* src_host,   /* nf device pointers [ncol][nlev][nt] */
                   const int* src_dtype_host,     /* nf entries, TEMX_F64 | TEMX_F32 */
                   double* const* acc_host,       /* nf device pointers [ncol][nlev] */
                   int64_t ncol, int nlev, int64_t nt,
                   int flags, void* stream);

/* TEMX_EINVAL: a null plan or pointer, nts < 1.  TEMX_ESTATE: temx_plan_set_tem has not been called.
 * TEMX_EUNSUPPORTED: M * nlev * nts >= 2^31.
 * results: [TEMX_NRESULTS][M][nlev][nts] fp64.  zonal_or_null: NULL or [TEMX_NZONAL][M][nlev][nts] fp64. */
int temxc_tem_from_zonal_means(temx_plan* plan,
                               double* zm8,       /* [8][M][nlev][nts]: slots 0..6 in, slot 7 scratch */
                               int64_t nts,
                               double* results, double* zonal_or_null, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_CLIM_H */
