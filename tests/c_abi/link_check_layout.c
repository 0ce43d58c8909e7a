/* Plain-C consumer of the third header: include/temx_layout.h must compile as C, its entry points must resolve
 * against libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_layout.h"

int main(void) {
  const void* src[1] = {(const void*)4096};
  void* dst[1] = {(void*)(1 << 20)};
  const int sdt[1] = {TEMX_F64};
  int rc = temxl_to_engine(0, 0, src, sdt, dst, TEMX_F64, 4, 3, 2, 0, 2, TEMXL_FLIP_LEV, 0);
  printf("temxl_version=%d nf0_rc=%d err=\"%s\"\n", temxl_version(), rc, temx_last_error());
  return (temxl_version() == 100 && rc == TEMX_EINVAL) ? 0 : 1;
}
