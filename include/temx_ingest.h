/* temx_ingest.h -- fourth header of libtemx.so: time-major model-level records to pressure levels in the engine's
 * layout, in one pass on the GPU.
 *
 * Native-grid model output is time-major and on hybrid levels at once: fields [time][lev][ncol] with ncol fastest and
 * ps [time][ncol].  temxi_records_to_pressure is temxl_to_engine (temx_layout.h) and temxv_interp in hybrid mode
 * (temx_vert.h) fused: every model-level element of the window is read once and every pressure-level element written
 * once, where the chain of the two writes and reads the model-level window again in between.  It needs no plan, so it
 * has a header, a prefix (temxi_) and a version of its own; the entry points of the other three headers and their
 * versions are untouched by it.
 *
 * Conventions are those of temx.h: device pointers unless the name ends in _host, dtype TEMX_F64 / TEMX_F32, stream a
 * hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h with the message in
 * temx_last_error().  method and edge take the TEMXV_* values of temx_vert.h.
 *
 * Contract of temxi_records_to_pressure:
 *   Result.  dst[f][i][j][t], i < ncol, j < nplev, t < ntb, is bit for bit -- every NaN included -- what temxv_interp
 *   (TEMXV_P_HYBRID, same method and edge, dtype = dst_dtype) returns on the output of temxl_to_engine (no flip,
 *   dst_dtype) for the window t0 .. t0 + ntb, with ps[t0 .. t0 + ntb) transposed to [ncol][ntb].  fp32 sources widen
 *   exactly; an fp64 source with dst_dtype TEMX_F32 is refused as in temxl_to_engine; the interpolation is carried out
 *   in fp64 and rounded once to dst_dtype.  Source pressure p = hyam[k] p0_hybrid + hybm[k] ps, levels top first.
 *   Bad columns, edges, ties.  As in temx_vert.h: a target equal to a level's pressure takes that level's value; a
 *   target outside the column follows edge; a (column, time) whose pressures are not finite and strictly increasing
 *   (TEMXV_LOG: or not all positive), or whose ps is not finite, is NaN at every target; a NaN field value reaches
 *   only the targets of its two brackets.
 *   Argument checks come before any device call and return TEMX_EINVAL with a message: nf outside 1..TEMXI_NF_MAX, a
 *   null pointer, sizes below 1 (nlev below 2), t0 < 0 or t0 + ntb > nt_src, plev not positive, finite and strictly
 *   ascending, a non-finite hyam, hybm or p0_hybrid, an unknown dtype, method or edge, a narrowing dtype, a pointer
 *   not aligned to its element size, a dst that overlaps a src, ps or another dst (a src is taken as its whole
 *   [nt_src][nlev][ncol] array, ps as its whole [nt_src][ncol] array).  A shape for which no tile or no single launch
 *   exists returns TEMX_EUNSUPPORTED before any launch.
 *   Launch behaviour.  Asynchronous and stream ordered.  The small tables (hyam, hybm, plev) go to the device through
 *   the cached upload temxv_interp uses: a call with tables seen before allocates nothing.  Nothing is written outside
 *   dst[f][0 .. ncol * nplev * ntb).  Two calls with the same arguments give the same bits.
 */
#ifndef TEMX_INGEST_H
#define TEMX_INGEST_H

#include <stdint.h>

#include "temx.h"
#include "temx_vert.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TEMXI_NF_MAX = 8 };

int temxi_version(void); /* 100 */

int temxi_records_to_pressure(int device, int nf,
                              const void* const* src_host,   /* nf device pointers [nt_src][nlev][ncol] */
                              const int* src_dtype_host,     /* nf entries, TEMX_F64 | TEMX_F32 */
                              void* const* dst_host,         /* nf device pointers [ncol][nplev][ntb] */
                              int dst_dtype,
                              int64_t ncol, int nlev, int64_t nt_src, int64_t t0, int64_t ntb,
                              int nplev, const double* plev_pa_host,
                              const double* hyam_host, const double* hybm_host, double p0_hybrid,
                              const void* ps, int ps_dtype,   /* [nt_src][ncol] */
                              int method, int edge,           /* TEMXV_LOG | TEMXV_LINEAR, TEMXV_EDGE_NAN | TEMXV_EDGE_HOLD */
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_INGEST_H */
