/* temx_tfilt.h -- eleventh header of libtemx.so: a finite-impulse-response filter along the time axis of fields in the
 * engine's layout ([ncol][nlev][nt], time fastest), the device step of the EP flux by time scale.  A band-passed record is
 * what a TEM run needs to give the eddy fluxes of one band of frequencies (synoptic transients, low-frequency
 * variability ...); the front end combines those fluxes with the mean state of the unfiltered run.
 *
 * The header has a prefix (temxf_) and a version of its own; the entry points of the other ten headers and their
 * versions are untouched.  Conventions are those of temx.h: stateless, device used as given, device pointers unless the
 * name ends in _host, dtype TEMX_F64 / TEMX_F32, stream a hipStream_t passed as void*, return value TEMX_OK or a negative
 * TEMX_E* code of temx.h with the message in temx_last_error().  Argument checks come before any device call.  The call
 * allocates nothing and is asynchronous and stream ordered.
 *
 * Contract of temxf_filter_time, per source field f, band b, row r = (column, level) and output time t in 0 .. nto,
 * nto = nt - nw + 1:
 *   dst[b][f][r][t] = round_dst( sum over k = 0 .. nw - 1 of w[b][k] * (double) src[f][r][t + k] )
 *   The sum is acc = fma(w[b][k], x, acc) with k ascending from acc = +0.0; fp32 sources widen exactly; there is one
 *   rounding to dst_dtype at the end.  The bits of an output are a fixed function of its nw inputs, the weights and the
 *   two dtypes: they do not depend on ncol, nlev, nt, nb, the row's position, the alignment of the pointers or how the
 *   launch is cut along rows or along time, and repeated calls are bitwise identical.  No atomics.  A non-finite input
 *   reaches the nw outputs of its own row whose window holds it and nothing else.  Nothing is written outside
 *   dst[b][f][0 .. ncol * nlev * nto).  The record is read once for all bands and written nb times.
 */
#ifndef TEMX_TFILT_H
#define TEMX_TFILT_H

#include <stdint.h>

#include "../../include/temx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TEMXF_NF_MAX = 8, TEMXF_NB_MAX = 4, TEMXF_NW_MAX = 255 };

int temxf_version(void); /* 100 */

/* nf in 1..TEMXF_NF_MAX fields and nb in 1..TEMXF_NB_MAX bands of nw weights each in one call; dst_host holds nb * nf
 * device pointers, band-major ([nb][nf]), each [ncol][nlev][nt - nw + 1] of dst_dtype.  flags: none is defined, pass 0.
 * TEMX_EINVAL: a null pointer; nf, nb or nw (1..TEMXF_NW_MAX) out of range; nw even; nt < nw; sizes below 1; an unknown
 * dtype or flag; an fp64 source with an fp32 destination (no call of this library narrows); a pointer not aligned to its
 * element size; a dst that overlaps a src, the weights or another dst.
 * TEMX_EUNSUPPORTED: a field needs 2^24 workgroups or more in one launch.  A workgroup takes 32 rows by a tile of at
 * least 64 output times (16 rows by 128 for fp64 sources with nw > 96, 8 rows by 256 with nw > 192; more rows where a
 * row has fewer than 64 outputs), so the limit lies at ncol * nlev * ceil(nto / tile) >= 2^29 and beyond: filter such
 * fields in parts along ncol. */
int temxf_filter_time(int device, int nf,
                      const void* const* src_host,   /* nf device pointers [ncol][nlev][nt] */
                      const int* src_dtype_host,     /* nf entries, TEMX_F64 | TEMX_F32 */
                      int nb,
                      void* const* dst_host,         /* [nb][nf] device pointers [ncol][nlev][nt - nw + 1] */
                      int dst_dtype,
                      int64_t ncol, int nlev, int64_t nt, int nw,
                      const double* weights,         /* device [nb][nw] */
                      int flags, void* stream);

/* How a launch over rows = ncol * nlev rows is cut, as seven ints: rows per workgroup rpb, output times per tile TT,
 * LDS elements per staged row (odd, >= TT + nw - 1), outputs per lane and run R, tiles along time, workgroups of one
 * field, bytes of the staged image.  src_esz and dst_esz are 4 or 8.  TEMX_EINVAL as above for the sizes;
 * TEMX_EUNSUPPORTED where temxf_filter_time would refuse the launch.  Needs no device. */
int temxf_filter_shape(int64_t rows, int64_t nt, int nw, int nb, int src_esz, int dst_esz, int* shape_host);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_TFILT_H */
