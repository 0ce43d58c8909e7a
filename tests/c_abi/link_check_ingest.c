/* Plain-C consumer of the fourth header: include/temx_ingest.h must compile as C, its entry points must resolve
 * against libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_ingest.h"

int main(void) {
  const void* src[1] = {(const void*)4096};
  void* dst[1] = {(void*)(1 << 20)};
  const int sdt[1] = {TEMX_F64};
  const double plev[2] = {5e4, 7e4}, hy[3] = {0.1, 0.2, 0.3};
  int rc = temxi_records_to_pressure(0, 0, src, sdt, dst, TEMX_F64, 4, 3, 5, 1, 2, 2, plev, hy, hy, 1e5,
                                     (const void*)(1 << 24), TEMX_F64, TEMXV_LOG, TEMXV_EDGE_NAN, 0);
  printf("temxi_version=%d nf_max=%d nf0_rc=%d err=\"%s\"\n", temxi_version(), (int)TEMXI_NF_MAX, rc, temx_last_error());
  return (temxi_version() == 100 && rc == TEMX_EINVAL) ? 0 : 1;
}
