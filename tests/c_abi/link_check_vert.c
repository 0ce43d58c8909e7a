/* Plain-C consumer of the second header: include/temx_vert.h must compile as C, its entry points must resolve
 * against libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_vert.h"

int main(void) {
  const double plev[2] = {50000.0, 70000.0};
  const double hy[3] = {0.1, 0.2, 0.3};
  const void* src[1] = {(const void*)4096};
  void* dst[1] = {(void*)(1 << 20)};
  int rc = temxv_interp(0, 0, src, dst, TEMX_F64, 4, 3, 2, 2, plev, TEMXV_P_HYBRID, hy, hy, 100000.0,
                        (const void*)(1 << 24), TEMX_F64, TEMXV_LOG, TEMXV_EDGE_NAN, 0);
  printf("temxv_version=%d nf0_rc=%d err=\"%s\"\n", temxv_version(), rc, temx_last_error());
  return (temxv_version() == 100 && rc == TEMX_EINVAL) ? 0 : 1;
}
