/* temx_gclim.h -- eighth header of libtemx.so: the device step of grouped and weighted time means (a monthly, seasonal
 * or yearly TEM climatology out of one record; monthly means weighted by the days of each month).
 *
 * A segmented, weighted sum over time of fields in the engine's layout ([ncol][nlev][nt], time fastest).  Every time of
 * the record carries a label (-1: left out, else the group 0 .. ng-1 it belongs to) and a weight; a call sums one block
 * of the record, the times t0 .. t0 + nt, into ng sums per row.  The sums are [ncol][nlev][ng], group fastest: the
 * engine's layout with nt = ng, so the group means go through the engine as ng snapshots.  The header has a prefix
 * (temxg_) and a version of its own; the entry points of the other seven headers and their versions are untouched.
 *
 * Conventions are those of temx.h: device pointers unless the name ends in _host, dtype TEMX_F64 / TEMX_F32, stream a
 * hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h with the message in
 * temx_last_error().  Argument checks come before any device call.  The call is asynchronous and stream ordered.  The
 * labels and weights of a record reach the device once (a table keyed by their content, never rewritten): every
 * further block of the record allocates nothing.
 *
 * Contract, per field f, row (i, k) and group g:
 *   acc[f][i][k][g] = sum over the times t of the block with label[t0 + t] == g of weight[t0 + t] * (double) src[f][i][k][t]
 *   (acc + sum under TEMXG_ACCUMULATE, one further rounding).  fp32 widens exactly, all arithmetic is fp64.  A (row,
 *   group) sum is a fixed function of the values, labels and weights of the block's times, of nt and of the source
 *   dtype: it does not depend on ncol, nlev, the row's position, the alignment of the pointers or the shape of the
 *   launch, so equal rows give equal bits and repeated calls are bitwise identical.  Sums start from -0.0: a group of
 *   one time with weight 1 is a bit copy of that element.  weight_host_or_null == NULL gives the bits of an array of
 *   ones.  A group with no time in the block is stored as zero without the flag; under the flag it keeps its bits and is
 *   neither read nor written.  A time labelled -1 never enters a sum, even if it is NaN; a weight of 0 still multiplies
 *   (0 * NaN poisons its group).  A non-finite value poisons its own (row, group) and nothing else.  No atomics: every
 *   output is stored once, by one lane.  Nothing is written outside acc[f][0 .. ncol * nlev * ng).
 */
#ifndef TEMX_GCLIM_H
#define TEMX_GCLIM_H

#include <stdint.h>

#include "temx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TEMXG_NF_MAX = 8, TEMXG_NG_MAX = 64 };
enum { TEMXG_ACCUMULATE = 1 };

int temxg_version(void); /* 100 */

/* nf in 1..TEMXG_NF_MAX fields in one call.  TEMX_EINVAL: nf or ng out of range, a null pointer (weights may be NULL),
 * an unknown dtype or flag, sizes below 1, a block that does not lie inside the record, a label outside -1..ng-1, a
 * weight that is negative or not finite, a pointer not aligned to its element size, an acc (ncol * nlev * ng
 * elements) that overlaps a src or another acc.  device is used as given.  TEMX_EUNSUPPORTED: a field needs 2^24
 * workgroups or more in one launch (as temxc_time_sum): sum such fields in parts along ncol. */
int temxg_time_sum_groups(int device, int nf,
                          const void* const* src_host,        /* nf device pointers [ncol][nlev][nt]: one block of the record */
                          const int* src_dtype_host,          /* nf entries, TEMX_F64 | TEMX_F32 */
                          double* const* acc_host,            /* nf device pointers [ncol][nlev][ng] */
                          int64_t ncol, int nlev, int64_t nt,
                          int64_t nt_record, int64_t t0,      /* the block holds times t0 .. t0 + nt of a record of nt_record */
                          int ng,
                          const int32_t* label_host,          /* nt_record labels: -1 left out, else 0 .. ng-1 */
                          const double* weight_host_or_null,  /* nt_record weights, finite and >= 0; NULL = all ones */
                          int flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_GCLIM_H */
