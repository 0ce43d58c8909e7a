/* temx_mtracer.h -- sixth header of libtemx.so: tracer TEM (Abalos et al. 2017) for fields with missing values.
 *
 * The temx_tracer_* entry points of temx.h are refused in missing-value mode (TEMX_OPT_MISSING = 1): a masked tracer
 * has a mask and a coverage of its own, and their signatures have no slot for it.  The two calls below are the masked
 * tracer run.  They have a header, a prefix (temxm_) and a version of their own; the entry points of temx.h,
 * temx_vert.h, temx_layout.h, temx_ingest.h and temx_clim.h and their versions are untouched.
 *
 * Conventions are those of temx.h: device pointers unless the name ends in _host, dtype TEMX_F64 / TEMX_F32, stream a
 * hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h with the message in
 * temx_last_error().  Argument and state checks come before any device call.  Workspace is allocated at the first call
 * and freed with the plan.
 *
 * Contract, per tracer q, on a plan in missing-value mode after a masked temx_tem_run on the same va, wap:
 *   Mask.  A point (i, d) is valid for the tracer when q, v and omega are all finite there -- the three arrays the run
 *     reads; u and T are not read.  The mask is the tracer's own: where the tracer is missing exactly where the fields
 *     are, it is the common mask of the TEM run.
 *   Fits.  qb is the masked fit of q under that mask: the functional, tau (TEMX_OPT_MISSING_WEIGHT) and basis of the
 *     masked mode of temx.h.  q' = q - qb(lat_i); v' and omega' are the eddies of the TEM run (its masked coefficients);
 *     q'v' and q'omega' are fitted under the tracer's mask, entering as 0 -- by a select -- where the point is not valid.
 *   Coverage.  tcov is the default operator applied to the tracer's validity indicator.  qb, qpvpb and qpwappb are NaN
 *     where it is below TEMX_OPT_MIN_COVERAGE, or where the column's system does not factor; the other three zonal
 *     arrays and the six results follow from them and from the zonal means of the TEM run by the tracer epilogue of
 *     temx_tracer_run, NaN spreading by IEEE propagation only.
 *   Native outputs.  qp, qpvp, qpwapp are NaN where the point is not valid for the tracer or the tracer's native
 *     coverage is below the threshold.
 *   Determinism and state.  No atomics: repeated calls are bitwise identical.  A tracer run changes nothing a later
 *     temx_tem_eddy, temx_get_matrix(TEMX_MAT_COVERAGE) or temx_tem_run on the plan returns.  The plan holds one
 *     tracer's coefficients at a time, as the unmasked path does.
 *   Limits.  Those of the masked mode: L <= 63, fp64 or fp32, q of the dtype of va and wap.
 */
#ifndef TEMX_MTRACER_H
#define TEMX_MTRACER_H

#include <stdint.h>

#include "temx.h"

#ifdef __cplusplus
extern "C" {
#endif

int temxm_version(void); /* 100 */

/* TEMX_EINVAL: a null plan, q, va, wap or tres; an unknown dtype.  TEMX_ESTATE: the plan is not in missing-value
 * mode, or no masked temx_tem_run since the last temx_plan_set_tem.
 * tres: [6][M][nlev][nt] fp64 = etfy etfz etdiv qtendetfd qtendvtem qtendwtem.
 * tzon_or_null: NULL or [6][M][nlev][nt] fp64 = qb qpvpb qpwappb dqb_dp qbcoslat dqbcoslat_dlat.
 * tcov_or_null: NULL or [M][nlev][nt] fp64, the tracer's coverage on the zonal grid. */
int temxm_tracer_run(temx_plan* plan, const void* q, const void* va, const void* wap, int dtype,
                     double* tres, double* tzon_or_null, double* tcov_or_null, void* stream);

/* The native fields of the tracer of the latest temxm_tracer_run: ptrs3_host holds three device pointers
 * (qp, qpvp, qpwapp), each [ncol][nlev][nt] fp64 or NULL.  TEMX_EINVAL and TEMX_ESTATE as above; TEMX_ESTATE also
 * when no temxm_tracer_run has followed the latest masked temx_tem_run. */
int temxm_tracer_eddy(temx_plan* plan, const void* q, const void* va, const void* wap, int dtype,
                      double* const* ptrs3_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_MTRACER_H */
