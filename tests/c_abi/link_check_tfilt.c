/* Plain-C consumer of the eleventh header: pytemdiags_amd/include/temx_tfilt.h must compile as C, its entry points must
 * resolve against libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_tfilt.h"

int main(void) {
  const void* src[1] = {(const void*)4096};
  const int dtype[1] = {TEMX_F64};
  void* dst[1] = {(void*)(1 << 20)};
  const double* w = (const double*)(1 << 24);
  int shape[7] = {0, 0, 0, 0, 0, 0, 0};
  int rc_even = temxf_filter_time(0, 1, src, dtype, 1, dst, TEMX_F64, 10, 2, 40, 4, w, 0, 0);       /* nw even */
  int rc_short = temxf_filter_time(0, 1, src, dtype, 1, dst, TEMX_F64, 10, 2, 4, 5, w, 0, 0);      /* nt < nw */
  int rc_narrow = temxf_filter_time(0, 1, src, dtype, 1, dst, TEMX_F32, 10, 2, 40, 5, w, 0, 0);    /* fp64 -> fp32 */
  int rc_null = temxf_filter_time(0, 1, src, dtype, 1, dst, TEMX_F64, 10, 2, 40, 5, 0, 0, 0);      /* null weights */
  int rc_shape = temxf_filter_shape(1000, 40, 9, 2, 8, 8, shape);
  printf("temxf_version=%d even_rc=%d short_rc=%d narrow_rc=%d null_rc=%d shape_rc=%d rpb=%d R=%d err=\"%s\"\n", temxf_version(),
         rc_even, rc_short, rc_narrow, rc_null, rc_shape, shape[0], shape[3], temx_last_error());
  /* the first header's version is untouched: temx_version() == 402 */
  printf("temx_version=%d (expected 402)\n", temx_version());
  return (temxf_version() == 100 && rc_even == TEMX_EINVAL && rc_short == TEMX_EINVAL && rc_narrow == TEMX_EINVAL &&
          rc_null == TEMX_EINVAL && rc_shape == TEMX_OK && shape[0] >= 1 && shape[3] >= 1 && TEMXF_NF_MAX == 8 &&
          TEMXF_NB_MAX == 4 && TEMXF_NW_MAX == 255 && temx_version() == 402) ? 0 : 1;
}
