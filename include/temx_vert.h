/* temx_vert.h -- second header of libtemx.so: model levels to pressure levels on the GPU.
 *
 * The TEM engine of temx.h takes fields on pressure levels (the reference has the same restriction,
 * tem_diagnostics.py:360-385).  Native model output lives on hybrid sigma-pressure levels, where
 * p = hyam p0 + hybm ps differs per column and time.  temxv_interp is the vertical remap in front of the engine.
 * It needs no plan (no grid, no basis), so it has a header, a prefix (temxv_) and a version of its own; the entry
 * points of temx.h and temx_version() are untouched by it.
 *
 * Conventions are those of temx.h: device pointers unless the name ends in _host, fields row-major
 * [ncol][nlev][nt] with time fastest, dtype TEMX_F64 / TEMX_F32, stream a hipStream_t passed as void*, return value
 * TEMX_OK or a negative TEMX_E* code of temx.h with the message in temx_last_error().  Argument checks come before
 * any device call.
 *
 * Contract of temxv_interp, per (column i, time t):
 *   source pressure   TEMXV_P_HYBRID  p[k] = hyam[k] * p0_hybrid + hybm[k] * ps[i][t], formed in fp64;
 *                                     ps_or_p is ps [ncol][nt] of type p_dtype, no 3-D pressure array is read
 *                     TEMXV_P_FIELD   p[k] = ps_or_p[i][k][t], an array [ncol][nlev][nt] of type p_dtype
 *                     model levels are top first: p increases with k.  plev_pa_host is strictly ascending, in Pa.
 *   method            TEMXV_LOG linear in ln p, TEMXV_LINEAR linear in p; weights and the blend in fp64, the
 *                     result rounded once to the field dtype
 *   edges             p_top = p[0], p_bot = p[nlev-1].  TEMXV_EDGE_NAN: a target outside [p_top, p_bot] is NaN.
 *                     TEMXV_EDGE_HOLD: above p_top the top value is held, between p_bot and the surface pressure
 *                     the bottom value is held, below the surface the result is NaN.  In field mode the surface
 *                     is p_bot: nothing below p_bot is held.
 *   bad columns       a (column, time) whose pressures are not strictly increasing, or not all finite, is NaN at
 *                     every target level.  With TEMXV_LOG so is one with a pressure <= 0 (interface levels
 *                     with p[0] = 0 have no ln p); TEMXV_LINEAR takes any finite increasing pressures.
 *                     A non-finite field value reaches only the targets whose bracket touches it.
 * Every input element is read once and every output element written once; src and dst are not copied or
 * re-laid out and must not overlap.  The call is asynchronous and stream ordered.  The small tables of a call (hyam,
 * hybm, plev) are uploaded once per distinct set and kept: the first call with a new set allocates and copies
 * synchronously, later calls with the same set touch no allocator (make that first call outside a graph capture).
 */
#ifndef TEMX_VERT_H
#define TEMX_VERT_H

#include <stdint.h>

#include "temx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TEMXV_P_HYBRID = 0, TEMXV_P_FIELD = 1 };
enum { TEMXV_LOG = 0, TEMXV_LINEAR = 1 };
enum { TEMXV_EDGE_NAN = 0, TEMXV_EDGE_HOLD = 1 };
enum { TEMXV_NF_MAX = 8 };

int temxv_version(void); /* 100 */

/* nf in 1..TEMXV_NF_MAX fields in one launch.  TEMX_EINVAL: nf out of range, a null pointer, sizes below 1
 * (nlev below 2) or out of range (nlev, nplev above 2^20, nt above 2^31, ncol above 2^40, or
 * ncol * max(nlev, nplev) * nt above 2^48, as in temx_layout.h, temx_ingest.h and temx_clim.h), plev not strictly
 * ascending or not positive, non-finite hyam / hybm / p0_hybrid, an unknown flag, a pointer not aligned to its element
 * size, a dst that overlaps a src, ps_or_p or another dst.  An array that would end beyond the top of the address space
 * is taken as reaching it in the overlap test, not as wrapping round.  hyam_host and hybm_host are read in hybrid mode
 * only (they may be NULL in field mode).  device is used as given.
 * The lane map is chosen by row length (rows of nt * itemsize below 128 bytes take the slab-staged map);
 * TEMXV_MAP=time or TEMXV_MAP=slab in the environment overrides the choice for A/B runs. */
int temxv_interp(int device, int nf,
                 const void* const* src_host, /* nf device pointers [ncol][nlev][nt]  */
                 void* const* dst_host,       /* nf device pointers [ncol][nplev][nt] */
                 int dtype, int64_t ncol, int nlev, int64_t nt,
                 int nplev, const double* plev_pa_host,
                 int pmode,                   /* TEMXV_P_HYBRID | TEMXV_P_FIELD */
                 const double* hyam_host, const double* hybm_host, double p0_hybrid,
                 const void* ps_or_p, int p_dtype,
                 int method,                  /* TEMXV_LOG | TEMXV_LINEAR */
                 int edge,                    /* TEMXV_EDGE_NAN | TEMXV_EDGE_HOLD */
                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_VERT_H */
