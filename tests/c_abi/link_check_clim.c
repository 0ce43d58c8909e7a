/* Plain-C consumer of the fifth header: include/temx_clim.h must compile as C, its entry points must resolve against
 * libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_clim.h"

int main(void) {
  const void* src[1] = {(const void*)4096};
  double* acc[1] = {(double*)(1 << 20)};
  const int sdt[1] = {TEMX_F64};
  double zm8[8] = {0}, res[TEMX_NRESULTS] = {0};
  int rc = temxc_time_sum(0, 0, src, sdt, acc, 4, 3, 2, TEMXC_ACCUMULATE, 0);
  int rp = temxc_tem_from_zonal_means(0, zm8, 1, res, 0, 0);
  printf("temxc_version=%d nf0_rc=%d null_plan_rc=%d err=\"%s\"\n", temxc_version(), rc, rp, temx_last_error());
  /* the first header's version is untouched: temx_version() == 402 */
  printf("temx_version=%d (expected 402)\n", temx_version());
  return (temxc_version() == 100 && rc == TEMX_EINVAL && rp == TEMX_EINVAL && temx_version() == 402) ? 0 : 1;
}
