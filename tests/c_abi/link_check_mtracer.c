/* Plain-C consumer of the sixth header: include/temx_mtracer.h must compile as C, its entry points must resolve against
 * libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_mtracer.h"

int main(void) {
  const void* f = (const void*)4096;
  double out[6] = {0};
  double* ptrs[3] = {out, out, out};
  int rr = temxm_tracer_run(0, f, f, f, TEMX_F64, out, 0, 0, 0);
  int re = temxm_tracer_eddy(0, f, f, f, TEMX_F64, ptrs, 0);
  printf("temxm_version=%d null_plan_run_rc=%d null_plan_eddy_rc=%d err=\"%s\"\n", temxm_version(), rr, re, temx_last_error());
  /* the first header's version is untouched: temx_version() == 402 */
  printf("temx_version=%d (expected 402)\n", temx_version());
  return (temxm_version() == 100 && rr == TEMX_EINVAL && re == TEMX_EINVAL && temx_version() == 402) ? 0 : 1;
}
