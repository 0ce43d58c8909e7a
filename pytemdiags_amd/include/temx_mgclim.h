/* temx_mgclim.h -- ninth header of libtemx.so: the device step of masked grouped time means (a monthly, seasonal or
 * day-weighted TEM climatology of fields with missing values).
 *
 * The grouped, weighted sum of temx_gclim.h taken over the valid times only, as the sum of temx_nclim.h takes them:
 * per field, row and group the weighted sum of the valid values, the sum of their weights and their number.  Fields are
 * in the engine's layout ([ncol][nlev][nt], time fastest); every time of the record carries a label (-1: left out, else
 * its group 0 .. ng-1) and a weight; a call sums one block of the record, the times t0 .. t0 + nt.  The outputs are
 * [ncol][nlev][ng], group fastest.  The header has a prefix (temxw_) and a version of its own; the entry points of the
 * other eight headers and their versions are untouched.  (The eight headers of ../../include are a closed set that the
 * tests of the grouped sum pin by name, so this one lives in the package's own include directory.)
 *
 * Conventions are those of temx.h: device pointers unless the name ends in _host, dtype TEMX_F64 / TEMX_F32, stream a
 * hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h with the message in
 * temx_last_error().  Argument checks come before any device call.  The call is asynchronous and stream ordered.  The
 * record's labels and weights reach the device once, in the table of temxg_time_sum_groups (keyed by content, shared
 * with it): every further block of the record allocates nothing.
 *
 * Contract, per field f, row (i, k) and group g; the sums run over the times t of the block with label[t0 + t] == g
 * that are valid:
 *   validity  an element is valid iff it is finite: NaN, +Inf and -Inf are missing.  Without TEMXW_COMMON_MASK every
 *             field has its own mask (and its own wsum and cnt); with it, time t of row (i, k) is valid iff it is valid
 *             in all nf fields, and the fields share wsum_host[0] and cnt_host[0].
 *   acc       the sum of weight * (double) src: one fp64 fma(w, x, a) per valid time, starting from -0.0.  fp32 widens
 *             exactly.
 *   wsum      the sum of the weights of the same times, a + w per step, in the same order.
 *   cnt       the number of those times, as a double, which is exact.
 *   missing   an invalid element never enters any arithmetic: a weight of 0 on an invalid time poisons nothing.  A time
 *             labelled -1 is never touched.  A (row, group) with no valid time gives sum zero (sign unspecified), wsum 0
 *             and cnt 0.
 *   absent    a group with no time in the block is stored as zero in all three outputs without TEMXW_ACCUMULATE; under
 *             the flag it is neither read nor written.
 *   TEMXW_ACCUMULATE  all three outputs are += with one further rounding; for cnt the result is exact.
 *   order     the order of the additions is that of temxg_time_sum_groups for the same block, labels, weights, t0 and
 *             dtype: acc equals by value its sums of the source with every invalid element replaced by +0.0
 *             (fma(w, 0, a) == a: only the sign of a zero can differ), wsum its sums of the indicator field of the same
 *             dtype (1 where valid under the applicable mask, else 0), cnt those with weights NULL.  So rows shorter
 *             than the plain time sum's switch (256 times fp64, 512 fp32) are added in ascending time in one
 *             accumulator; longer rows by lane l of a wave over the times l + 64 i, i ascending, and then in the order
 *             of the butterfly over the 64 lanes.
 *   reproducibility   results do not depend on ncol, nlev, the row's position, the alignment of the pointers beyond
 *             the element size, the shape of the launch or which form of the kernel ran (the groups present in the
 *             block and nf pick the form and no bit).  In own-mask mode a field's results do not depend on what else
 *             the call carries.
 *   memory    no atomics.  Every output is stored once, by one lane.  Nothing is written outside acc[f], wsum[..] and
 *             cnt[..][0 .. ncol * nlev * ng).
 *   reads     every source element is read from HBM once, with one exception: long rows with more groups present than
 *             one wave's LDS image holds (64 KiB / ((fields of a workgroup + 2) * 512 bytes): 12 groups for 8 fields
 *             under a common mask, 21 for 4, 42 for one) take the groups present in batches of that size and walk the
 *             row once per batch; the passes after the first re-read the row, from L2 where it stays.  The cut into
 *             batches changes no bit: every (row, group) sum is formed inside one pass.
 */
#ifndef TEMX_MGCLIM_H
#define TEMX_MGCLIM_H

#include <stdint.h>

#include "../../include/temx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TEMXW_NF_MAX = 8, TEMXW_NG_MAX = 64 };
enum { TEMXW_ACCUMULATE = 1, TEMXW_COMMON_MASK = 2 };

int temxw_version(void); /* 100 */

/* nf in 1..TEMXW_NF_MAX fields of one dtype in one call.  TEMX_EINVAL: nf or ng out of range, a null pointer (weights
 * may be NULL; a wsum_host[f] or cnt_host[f] that is used counts), an unknown dtype or flag, sizes below 1, a block that
 * does not lie inside the record, a label outside -1..ng-1, a weight that is negative or not finite, a pointer not
 * aligned to its element size, an output (ncol * nlev * ng elements) that overlaps a src or another output.  device is
 * used as given.  TEMX_EUNSUPPORTED: the call needs 2^24 workgroups or more in one launch (as temxn_time_sum_valid and
 * temxg_time_sum_groups): sum such fields in parts along ncol. */
int temxw_time_sum_groups_valid(int device, int nf,
                                const void* const* src_host,        /* nf device pointers [ncol][nlev][nt]: one block of the record */
                                int src_dtype,                      /* TEMX_F64 | TEMX_F32, one for the call */
                                double* const* acc_host,            /* nf device pointers [ncol][nlev][ng] */
                                double* const* wsum_host,           /* nf device pointers [ncol][nlev][ng]; under
                                                                       TEMXW_COMMON_MASK only wsum_host[0] is used */
                                double* const* cnt_host,            /* same rule */
                                int64_t ncol, int nlev, int64_t nt,
                                int64_t nt_record, int64_t t0,      /* the block holds times t0 .. t0 + nt of a record of nt_record */
                                int ng,
                                const int32_t* label_host,          /* nt_record labels: -1 left out, else 0 .. ng-1 */
                                const double* weight_host_or_null,  /* nt_record weights, finite and >= 0; NULL = all ones */
                                int flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_MGCLIM_H */
