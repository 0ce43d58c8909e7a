/* temx_wave.h -- tenth header of libtemx.so: zonal wavenumbers on an unstructured grid.  The wave-m component of a
 * field, its amplitude and phase, and the wave-m eddy fluxes u'v', u'omega', v'theta' on the zonal grid -- "which waves
 * carry the Eliassen-Palm flux" -- without a remap to a lat-lon grid and an FFT along longitude.
 *
 * The header has a prefix (temxk_) and a version of its own; the entry points of the other nine headers and their
 * versions are untouched.  Conventions are those of temx.h: device pointers unless the name ends in _host, dtype
 * TEMX_F64 / TEMX_F32, stream a hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h
 * with the message in temx_last_error().  Argument checks come before any device call.  The compute calls are
 * asynchronous and stream ordered.
 *
 * Contract.  Columns i with lat_i (the plan's) and lon_i, L and the output latitudes phi_j (j < M) of the plan.
 *   basis   for a zonal wavenumber m in 1..L and l = m..L (ndeg = L + 1 - m degrees, Kc = 2 ndeg columns)
 *             Pbar_l^m(x) = sqrt(2) sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) P_l^m(x),   x = sin(lat),
 *           P_l^m with the Condon-Shortley phase (scipy.special.lpmv(m, l, x)); column l - m of Ym [N][Kc] is
 *           Pbar_l^m(sin lat_i) cos(m lon_i), column ndeg + l - m the same with sin.
 *   fit     per field x and column d of [nlev][nt]:  c_m = argmin_c || Ym c - x' ||, unweighted, over every column of
 *           the grid, on the EDDY x' = x - Y0 pinv(Y0) x of the plan's zonal mean (on a cubed sphere Ym^T Y0 is far
 *           from zero for m = 4, 8, ...: a fit of the raw field would put part of the zonal mean into those waves).
 *           Each wavenumber is fitted on its own.  coef [Kc][D]: the cos half a_l, then the sin half b_l.
 *   zonal   Xc(j, d) = sum_l a_l(d) Pbar_l^m(sin phi_j), Xs the same with b_l: the wave-m component of the field is
 *           x'_m(phi, lambda) = Xc cos(m lambda) + Xs sin(m lambda); amplitude sqrt(Xc^2 + Xs^2), phase
 *           atan2(Xs, Xc) / m (the longitude of the ridge, radians).
 *   fluxes  the zonal mean of the product of two wave-m components, [x'_m y'_m] = (Xc Yc + Xs Ys) / 2, for (u, v),
 *           (u, omega), (v, theta), theta = T (p0/p)^kappa as in temx_tem_run.
 *   The sum of the fluxes over m is NOT the total eddy flux of temx_tem_run: noise and the leakage between m and m +- 4
 *   on a cubed sphere stay outside (the zonal mean, m = 0, has the same property in the reference).
 *
 * How it runs.  At temxk_wave_create the basis of every wavenumber is built on the device, deflated by the plan's own
 * native zonal-mean operator (Ymd = Ym - Y0 pinv(Y0) Ym, so that Ymd^T x = Ym^T x'), stored as the 4x4 blocks the
 * projection sweep streams (ncol x Kc x 8 bytes per wavenumber, up to the padding), and Gm = Ym^T Ym is factorised on
 * the host (Cholesky, fp64).  A call then reads the fields ONCE per wavenumber whose Kc is at most 128 (once per 128
 * columns of basis beyond that): the zonal-mean coefficients of the fields are not needed.  Everything is deterministic
 * -- no atomics, fixed reduction order, repeated calls are bitwise identical -- and nothing is written outside the
 * outputs; workspace is owned by the wave state.  No call changes plan state that a later call on the plan can see.
 */
#ifndef TEMX_WAVE_H
#define TEMX_WAVE_H

#include <stdint.h>

#include "../../include/temx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct temxk_wave temxk_wave;

enum { TEMXK_NF_MAX = 8, TEMXK_NM_MAX = 64, TEMXK_KC_MAX = 512 };

int temxk_version(void); /* 100 */

/* The wave state of nm distinct wavenumbers on a finalised plan (TEMX_ESTATE otherwise); it uses the plan, which must
 * outlive it.  TEMX_EINVAL: a null pointer, nm outside 1..TEMXK_NM_MAX, an m outside 1..L, a wavenumber given twice, a
 * longitude that is not finite.  TEMX_EUNSUPPORTED: Kc = 2 (L + 1 - m) > TEMXK_KC_MAX, and a plan in weights mode, in
 * missing-value mode, on latitude bins or finalised with a Gram matrix from outside (an ncol-sharded job).
 * TEMX_ERANK, with m in the message: Gm is not positive definite (the grid does not resolve wavenumber m at degree L).
 * The rule: a pivot of the Cholesky factorisation of Gm [Kc][Kc] at or below Kc 2^-52 max_j Gm[j][j] is refused -- it
 * lies inside the rounding of the sums that make Gm.  It is relative to the LARGEST diagonal entry: on a lat-lon grid of
 * nlon longitudes sin(m lon) at m = nlon / 2 is 1e-16 in every column, orthogonal to the cos half, and its pivots are
 * 1e-29 of the others (refused), while at m = nlon / 2 - 1 the smallest pivot is 0.9 of the largest diagonal entry.  No
 * state is made (*out stays null) and the plan is as before the call.
 * The call runs the plan's own temx_zonal_mean once per wavenumber on Kc columns (the deflation): the plan's operator
 * workspace may grow to that width; no result of the plan and none of its TEM state changes. */
int temxk_wave_create(temxk_wave** out, temx_plan* plan, const double* lon_deg_host /* [ncol] */, int nm,
                      const int* m_host /* [nm] */);
void temxk_wave_destroy(temxk_wave* wave);

/* device bytes the wave state holds now: the stored bases, the tables and the workspace of the calls so far */
int64_t temxk_wave_workspace_bytes(const temxk_wave* wave);

/* The operator alone, for wavenumber m_host[mi]: Xc and Xs of nf in 1..TEMXK_NF_MAX fields [ncol][D] (no theta
 * scaling), parts [nf][2][M][D], and on request the coefficients coef [nf][Kc][D].  TEMX_EINVAL: a null pointer, mi or
 * nf out of range, an unknown dtype, D outside [1, 2^28). */
int temxk_wave_project(temxk_wave* wave, int mi, int nf, const void* const* fields_host, const int* dtype_host,
                       int64_t D, double* parts, double* coef_or_null, void* stream);

/* The three wave-m fluxes of every wavenumber of the state, flux [nm][3][M][nlev][nt] in the order u'v', u'omega',
 * v'theta', and on request the parts of u, v, theta, omega, parts [nm][4][2][M][nlev][nt].  Needs temx_plan_set_tem
 * (TEMX_ESTATE otherwise); the fields are those of temx_tem_run.  TEMX_EUNSUPPORTED when the plan has been put into
 * missing-value mode or on latitude bins since the state was made. */
int temxk_wave_fluxes(temxk_wave* wave, const void* ua, const void* va, const void* ta, const void* wap, int dtype,
                      double* flux, double* parts_or_null, void* stream);

/* Synchronises the stream and reports whether a non-finite value reached the sums of temxk_wave_project or
 * temxk_wave_fluxes since the last call (the counterpart of temx_status, with a flag of the wave state's own: neither
 * call sees the other's sums).  Without this call a non-finite input goes unreported: it comes out as NaN. */
int temxk_wave_status(temxk_wave* wave, int* nonfinite_host, void* stream);

/* How the basis of wavenumber m at truncation L (1 <= m <= L <= 511, TEMX_EINVAL otherwise) is stored and swept, as six
 * ints: degrees L + 1 - m, Kc, sweeps over the fields per call, 4x4 blocks of the last sweep, blocks stored per group of
 * four rows, stored columns (4 x that; the stored basis is ncol rounded up to 16, times this, times 8 bytes).  Needs no
 * device and no state. */
int temxk_wave_shape(int L, int m, int* shape6_host);

/* ---- measurement helpers (tools/wave_bench.py; not on the product path) ----
 * HIP events around the projection sweeps (sweep + slab reduction, one pair per wavenumber) of temxk_wave_fluxes, on the
 * call's stream.  temxk_wave_timing(enable) switches them on or off and drops what was recorded; temxk_wave_timing_read
 * synchronises the recorded events and returns the sum of their durations and their number. */
int temxk_wave_timing(temxk_wave* wave, int enable);
int temxk_wave_timing_read(temxk_wave* wave, double* sum_ms_host, int* launches_host);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_WAVE_H */
