/* Plain-C consumer of the twelfth header: pytemdiags_amd/include_wavecls/temx_wavecls.h must compile as C, its entry points
 * must resolve against libtemx.so, and argument checks come before any device call.  No GPU needed. */
#include <stdio.h>
#include "temx_wavecls.h"

int main(void) {
  temxz_wave* w = (temxz_wave*)4096;
  const double lon[2] = {0.0, 90.0};
  const int m[1] = {1};
  const void* fields[1] = {(const void*)4096};
  const int dtype[1] = {TEMX_F64};
  double* out = (double*)(1 << 20);
  int shape[5] = {0, 0, 0, 0, 0}, launch[4] = {0, 0, 0, 0}, flag = 0;
  int rc_create = temxz_wave_create(&w, 0, lon, 1, m);                 /* null plan */
  int rc_null = temxz_wave_create(0, 0, lon, 1, m);
  int rc_project = temxz_wave_project(0, 0, 1, fields, dtype, 6, out, 0, 0);
  int rc_fluxes = temxz_wave_fluxes(0, fields[0], fields[0], fields[0], fields[0], TEMX_F64, out, 0, 0);
  int rc_status = temxz_wave_status(0, &flag, 0);
  int rc_launch = temxz_wave_launch(0, 0, 4, 6, launch);
  int rc_wide = temxz_wave_shape(65, 1, shape);                        /* 65 degrees: the generic form's */
  int rc_shape = temxz_wave_shape(50, 1, shape);
  long long bytes = (long long)temxz_wave_workspace_bytes(0);
  temxz_wave_destroy(0);
  printf("temxz_version=%d create_rc=%d project_rc=%d fluxes_rc=%d bytes=%lld shape=%d,%d,%d,%d,%d err=\"%s\"\n", temxz_version(),
         rc_create, rc_project, rc_fluxes, bytes, shape[0], shape[1], shape[2], shape[3], shape[4], temx_last_error());
  /* the first header's version is untouched: temx_version() == 402 */
  printf("temx_version=%d (expected 402)\n", temx_version());
  return (temxz_version() == 100 && rc_create == TEMX_EINVAL && rc_null == TEMX_EINVAL && w == 0 && rc_project == TEMX_EINVAL &&
          rc_fluxes == TEMX_EINVAL && rc_status == TEMX_EINVAL && rc_launch == TEMX_EINVAL && rc_shape == TEMX_OK &&
          rc_wide == TEMX_EUNSUPPORTED && bytes == 0 && shape[0] == 50 && shape[1] == 100 && shape[2] == 7 && shape[3] == 28 &&
          shape[4] == 1 && TEMXZ_NF_MAX == 8 && TEMXZ_NM_MAX == 64 && TEMXZ_NDEG_MAX == 64 && temx_version() == 402) ? 0 : 1;
}
