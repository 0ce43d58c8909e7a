/* Plain-C consumer of the tenth header: pytemdiags_amd/include/temx_wave.h must compile as C, its entry points must
 * resolve against libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_wave.h"

int main(void) {
  temxk_wave* w = (temxk_wave*)4096;
  const double lon[2] = {0.0, 90.0};
  const int m[1] = {1};
  const void* fields[1] = {(const void*)4096};
  const int dtype[1] = {TEMX_F64};
  double* out = (double*)(1 << 20);
  int rc_create = temxk_wave_create(&w, 0, lon, 1, m);                 /* null plan */
  int rc_null = temxk_wave_create(0, 0, lon, 1, m);
  int rc_project = temxk_wave_project(0, 0, 1, fields, dtype, 6, out, 0, 0);
  int rc_fluxes = temxk_wave_fluxes(0, fields[0], fields[0], fields[0], fields[0], TEMX_F64, out, 0, 0);
  long long bytes = (long long)temxk_wave_workspace_bytes(0);
  temxk_wave_destroy(0);
  printf("temxk_version=%d create_rc=%d project_rc=%d fluxes_rc=%d bytes=%lld err=\"%s\"\n", temxk_version(), rc_create,
         rc_project, rc_fluxes, bytes, temx_last_error());
  /* the first header's version is untouched: temx_version() == 402 */
  printf("temx_version=%d (expected 402)\n", temx_version());
  return (temxk_version() == 100 && rc_create == TEMX_EINVAL && rc_null == TEMX_EINVAL && w == 0 && rc_project == TEMX_EINVAL &&
          rc_fluxes == TEMX_EINVAL && bytes == 0 && TEMXK_NF_MAX == 8 && TEMXK_NM_MAX == 64 && TEMXK_KC_MAX == 512 &&
          temx_version() == 402) ? 0 : 1;
}
