/* Plain-C consumer of the eighth header: include/temx_gclim.h must compile as C, its entry points must resolve against
 * libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_gclim.h"

int main(void) {
  const void* src[1] = {(const void*)4096};
  double* acc[1] = {(double*)(1 << 20)};
  const int dt[1] = {TEMX_F64};
  const int32_t label[5] = {0, 1, -1, 1, 0};
  const double weight[5] = {1.0, 0.5, 3.0, 2.0, 0.25};
  int rc0 = temxg_time_sum_groups(0, 0, src, dt, acc, 4, 3, 2, 5, 1, 2, label, weight, TEMXG_ACCUMULATE, 0);
  int rc65 = temxg_time_sum_groups(0, 1, src, dt, acc, 4, 3, 2, 5, 1, 65, label, 0, 0, 0);
  printf("temxg_version=%d nf0_rc=%d ng65_rc=%d err=\"%s\"\n", temxg_version(), rc0, rc65, temx_last_error());
  /* the first header's version is untouched: temx_version() == 402 */
  printf("temx_version=%d (expected 402)\n", temx_version());
  return (temxg_version() == 100 && rc0 == TEMX_EINVAL && rc65 == TEMX_EINVAL && TEMXG_NF_MAX == 8 && TEMXG_NG_MAX == 64 &&
          temx_version() == 402) ? 0 : 1;
}
