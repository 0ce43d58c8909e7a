/* Plain-C consumer of the seventh header: include/temx_nclim.h must compile as C, its entry points must resolve against
 * libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_nclim.h"

int main(void) {
  const void* src[1] = {(const void*)4096};
  double* acc[1] = {(double*)(1 << 20)};
  double* cnt[1] = {(double*)(1 << 21)};
  int rc = temxn_time_sum_valid(0, 0, src, TEMX_F64, acc, cnt, 4, 3, 2, TEMXN_ACCUMULATE | TEMXN_COMMON_MASK, 0);
  printf("temxn_version=%d nf0_rc=%d err=\"%s\"\n", temxn_version(), rc, temx_last_error());
  /* the first header's version is untouched: temx_version() == 402 */
  printf("temx_version=%d (expected 402)\n", temx_version());
  return (temxn_version() == 100 && rc == TEMX_EINVAL && TEMXN_NF_MAX == 8 && temx_version() == 402) ? 0 : 1;
}
