/* temx_layout.h -- third header of libtemx.so: time-major records to the engine's layout on the GPU.
 *
 * Model output arrives time-major, [time][lev][ncol] with ncol fastest; the engine of temx.h works on
 * [ncol][lev][time] with time fastest.  temxl_to_engine is the re-layout in front of the engine: it moves a window
 * of snapshots of up to TEMXL_NF_MAX fields in one launch, each element read once and written once.  It needs no
 * plan, so it has a header, a prefix (temxl_) and a version of its own; the entry points of temx.h and temx_vert.h
 * and their versions are untouched by it.
 *
 * Conventions are those of temx.h: device pointers unless the name ends in _host, dtype TEMX_F64 / TEMX_F32, stream a
 * hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h with the message in
 * temx_last_error().  Argument checks come before any device call.
 *
 * Contract of temxl_to_engine, per field f, column i, level k, time t of the window:
 *   dst[f][i][k'][t] = (dst_dtype) src[f][t0 + t][k][i],   k' = nlev - 1 - k under TEMXL_FLIP_LEV, k' = k otherwise
 *   a move between equal dtypes is a bit copy (NaN payloads and -0.0 survive); fp32 -> fp64 widens; fp64 -> fp32 is
 *   refused.  nlev >= 1 (this is a layout call, not a TEM call).  Nothing is written outside
 *   dst[f][0 .. ncol * nlev * ntb).  The call is asynchronous and stream ordered and allocates nothing.
 */
#ifndef TEMX_LAYOUT_H
#define TEMX_LAYOUT_H

#include <stdint.h>

#include "temx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { TEMXL_NF_MAX = 8 };
enum { TEMXL_FLIP_LEV = 1 };

int temxl_version(void); /* 100 */

/* nf in 1..TEMXL_NF_MAX fields in one launch.  TEMX_EINVAL: nf out of range, a null pointer, an unknown dtype or a
 * narrowing one (an fp64 source with dst_dtype TEMX_F32), sizes below 1, t0 < 0, t0 + ntb > nt_src, an unknown
 * flag, a pointer not aligned to its element size, a dst that overlaps a src or another dst (a src is taken as its
 * whole [nt_src][nlev][ncol] array).  device is used as given. */
int temxl_to_engine(int device, int nf,
                    const void* const* src_host,   /* nf device pointers [nt_src][nlev][ncol] */
                    const int* src_dtype_host,     /* nf entries, TEMX_F64 | TEMX_F32 */
                    void* const* dst_host,         /* nf device pointers [ncol][nlev][ntb] */
                    int dst_dtype,
                    int64_t ncol, int nlev, int64_t nt_src, int64_t t0, int64_t ntb,
                    int flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_LAYOUT_H */
