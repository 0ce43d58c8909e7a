/* temx_nclim.h -- seventh header of libtemx.so: the time sum over the valid times of fields with missing values, the
 * device step of a time-mean TEM in missing-value mode (a masked climatology).
 *
 * temxc_time_sum of temx_clim.h propagates a non-finite value into its row.  A time mean over a mask that varies in
 * time needs, per (column, level), the sum over the valid times of each field and the number of valid times, with
 * every element read once.  That step has a header, a prefix (temxn_) and a version of its own; the entry points of
 * temx.h, temx_vert.h, temx_layout.h, temx_ingest.h, temx_clim.h and temx_mtracer.h and their versions are untouched.
 *
 * Conventions are those of temx.h: device pointers unless the name ends in _host, dtype TEMX_F64 / TEMX_F32, stream a
 * hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h with the message in
 * temx_last_error().  Argument checks come before any device call.  The call is asynchronous and stream ordered and
 * allocates nothing.
 *
 * Contract of temxn_time_sum_valid, per field f, column i, level k:
 *   validity  an element is valid iff it is finite: NaN, +Inf and -Inf are missing.  Without TEMXN_COMMON_MASK every
 *             field has its own mask; with it, time t of row (i, k) is valid iff it is valid in all nf fields.
 *   sums      acc[f][i][k] = sum over the valid t of (double) src[f][i][k][t].  fp32 widens exactly, every addition is
 *             fp64.  A non-finite value never reaches acc.
 *   counts    cnt[f][i][k] (cnt[0][i][k] under TEMXN_COMMON_MASK, the one count all fields share) = the number of valid
 *             times, as a double, which is exact.  A row with no valid time gives sum zero (sign unspecified) and
 *             count 0.
 *   TEMXN_ACCUMULATE  acc and cnt are += with one further rounding; for cnt the result is exact.
 *   reproducibility   the sum of a row is a fixed function of its values, the mask, nt, the dtype and the flags; in
 *             common-mask mode it may also depend on nf.  It never depends on ncol, nlev, the row's position, the
 *             alignment of the pointers beyond the element size or the shape of the launch: equal rows give equal
 *             bits, repeated calls are bitwise identical.  In own-mask mode the sum does not depend on what else the
 *             call carries.  A row of one valid element comes out bit for bit.
 *   memory    no atomics.  Nothing is written outside acc[f][0 .. ncol * nlev) and cnt[..][0 .. ncol * nlev).
 */
#ifndef TEMX_NCLIM_H
#define TEMX_NCLIM_H

#include <stdint.h>

#include "temx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TEMXN_NF_MAX = 8 };
enum { TEMXN_ACCUMULATE = 1, TEMXN_COMMON_MASK = 2 };

int temxn_version(void); /* 100 */

/* nf in 1..TEMXN_NF_MAX fields of one dtype in one call.  TEMX_EINVAL: nf out of range, a null pointer (a cnt_host[f]
 * that is used included), an unknown dtype or flag, sizes below 1, a pointer not aligned to its element size, an acc
 * or cnt that overlaps a src or another acc or cnt.  device is used as given.  TEMX_EUNSUPPORTED: the call needs 2^24
 * workgroups or more in one launch -- rows too long to stage take one wave each, four to a workgroup, so the limit
 * there is ncol * nlev >= 2^26 rows; shorter rows go at least 16 to a workgroup.  Sum such fields in parts along
 * ncol. */
int temxn_time_sum_valid(int device, int nf,
                         const void* const* src_host,   /* nf device pointers [ncol][nlev][nt] */
                         int src_dtype,                 /* TEMX_F64 | TEMX_F32, one for the call */
                         double* const* acc_host,       /* nf device pointers [ncol][nlev] */
                         double* const* cnt_host,       /* nf device pointers [ncol][nlev]; under
                                                           TEMXN_COMMON_MASK only cnt_host[0] is used */
                         int64_t ncol, int nlev, int64_t nt, int flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_NCLIM_H */
