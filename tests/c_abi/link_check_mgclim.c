/* Plain-C consumer of the ninth header: pytemdiags_amd/include/temx_mgclim.h must compile as C, its entry points must
 * resolve against libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_mgclim.h"

int main(void) {
  const void* src[1] = {(const void*)4096};
  double* acc[1] = {(double*)(1 << 20)};
  double* wsum[1] = {(double*)(2 << 20)};
  double* cnt[1] = {(double*)(3 << 20)};
  const int32_t label[5] = {0, 1, -1, 1, 0};
  const double weight[5] = {1.0, 0.5, 3.0, 2.0, 0.25};
  int rc0 = temxw_time_sum_groups_valid(0, 0, src, TEMX_F64, acc, wsum, cnt, 4, 3, 2, 5, 1, 2, label, weight,
                                        TEMXW_ACCUMULATE | TEMXW_COMMON_MASK, 0);
  int rc65 = temxw_time_sum_groups_valid(0, 1, src, TEMX_F64, acc, wsum, cnt, 4, 3, 2, 5, 1, 65, label, 0, 0, 0);
  printf("temxw_version=%d nf0_rc=%d ng65_rc=%d err=\"%s\"\n", temxw_version(), rc0, rc65, temx_last_error());
  /* the first header's version is untouched: temx_version() == 402 */
  printf("temx_version=%d (expected 402)\n", temx_version());
  return (temxw_version() == 100 && rc0 == TEMX_EINVAL && rc65 == TEMX_EINVAL && TEMXW_NF_MAX == 8 && TEMXW_NG_MAX == 64 &&
          TEMXW_ACCUMULATE == 1 && TEMXW_COMMON_MASK == 2 && temx_version() == 402) ? 0 : 1;
}
