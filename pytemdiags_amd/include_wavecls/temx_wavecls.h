/* temx_wavecls.h -- twelfth header of libtemx.so: the class form of the zonal-wavenumber fit.  The same fit, wave-m
 * components and wave-m eddy fluxes as temx_wave.h, for grids whose columns share latitudes (a cubed sphere, a lat-lon or
 * Gaussian grid): the matrix work is done once per latitude class instead of once per column, and the state keeps a few
 * bytes per column instead of a deflated basis of Kc columns.  Opt-in: nothing selects it automatically.
 *
 * The header has a prefix (temxz_) and a version of its own; the entry points of the other eleven headers and their
 * versions are untouched.  Conventions are those of temx.h: device pointers unless the name ends in _host, dtype
 * TEMX_F64 / TEMX_F32, stream a hipStream_t passed as void*, return value TEMX_OK or a negative TEMX_E* code of temx.h
 * with the message in temx_last_error().  Argument checks come before any device call.  The compute calls are
 * asynchronous and stream ordered.
 *
 * Contract: that of temx_wave.h, restated.  Columns i with lat_i (the plan's) and lon_i, L and the output latitudes
 * phi_j (j < M) of the plan.
 *   basis   for a zonal wavenumber m in 1..L and l = m..L (ndeg = L + 1 - m degrees, Kc = 2 ndeg columns)
 *             Pbar_l^m(x) = sqrt(2) sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) P_l^m(x),   x = sin(lat),
 *           P_l^m with the Condon-Shortley phase (scipy.special.lpmv(m, l, x)); column l - m of Ym [N][Kc] is
 *           Pbar_l^m(sin lat_i) cos(m lon_i), column ndeg + l - m the same with sin.
 *   fit     per field x and column d of [nlev][nt]:  c_m = argmin_c || Ym c - x' ||, unweighted, over every column of
 *           the grid, on the EDDY x' = x - Y0 pinv(Y0) x of the plan's zonal mean.  Each wavenumber is fitted on its
 *           own.  coef [Kc][D]: the cos half a_l, then the sin half b_l.
 *   zonal   Xc(j, d) = sum_l a_l(d) Pbar_l^m(sin phi_j), Xs the same with b_l; amplitude sqrt(Xc^2 + Xs^2), phase
 *           atan2(Xs, Xc) / m.
 *   fluxes  [x'_m y'_m] = (Xc Yc + Xs Ys) / 2 for (u, v), (u, omega), (v, theta), theta = T (p0/p)^kappa as in
 *           temx_tem_run.
 * The one difference: in the sums Ym^T x' a member's basis row is evaluated at the latitude of its CLASS, the mean |lat|
 * of the members, which lies within the plan's class tolerance (1e-11 degrees, 1e-8 for a plan made for fp32 fields) of
 * the member's own; the Gram matrix Ym^T Ym is that of temx_wave.h.
 *
 * How it runs.  Columns of one class side share Pbar_l^m(sin lat) and their row Z_s [Kc] of P Ym, P = Y0 pinv(Y0) the
 * plan's native zonal-mean operator, so per field and column d
 *     (Ym - P Ym)^T x = sum over class sides s of  Pbar(lat_s) (x) [sum_i x_i cos(m lon_i), sum_i x_i sin(m lon_i)]
 *                                                  - Z_s sum_i x_i
 * -- three fused multiply-adds per element and, per group of four classes, three small matrix products per block of
 * four coefficients.  At create the state is built as in temx_wave.h (the basis, its Gram matrix with the same Cholesky
 * factorisation and rank rule, P Ym by the plan's own temx_zonal_mean); then the class tables are gathered and everything
 * of size ncol x Kc is freed.  What stays per wavenumber: 16 bytes of weights per entry of the plan's row table, the class
 * basis and the two deflation tables (10 x 128 bytes per class-group and block of degrees).  A call reads the fields ONCE
 * per wavenumber.  Everything is deterministic -- no atomics, fixed reduction order, repeated calls are bitwise identical
 * -- and nothing is written outside the outputs; workspace is owned by the state.  No call changes plan state that a later
 * call on the plan can see.
 */
#ifndef TEMX_WAVECLS_H
#define TEMX_WAVECLS_H

#include <stdint.h>

#include "../../include/temx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct temxz_wave temxz_wave;

enum { TEMXZ_NF_MAX = 8, TEMXZ_NM_MAX = 64, TEMXZ_NDEG_MAX = 64 };

int temxz_version(void); /* 100 */

/* The class-form state of nm distinct wavenumbers on a finalised plan (TEMX_ESTATE otherwise); it uses the plan, which
 * must outlive it.  TEMX_EINVAL: a null pointer, nm outside 1..TEMXZ_NM_MAX, an m outside 1..L, a wavenumber given
 * twice, a longitude that is not finite.  TEMX_EUNSUPPORTED: a plan without latitude-class tables (a grid without
 * repeated latitudes, a plan made without classes), ndeg = L + 1 - m > TEMXZ_NDEG_MAX (wider bases stay with
 * temx_wave.h), and a plan in weights mode, in missing-value mode, on latitude bins or finalised with a Gram matrix from
 * outside.  TEMX_ERANK, with m in the message: the Gram matrix of the basis is not positive definite (the rule of
 * temx_wave.h).  No state is made (*out stays null) and the plan is as before the call.
 * The call runs the plan's own temx_zonal_mean once per wavenumber on Kc columns: the plan's operator workspace may grow
 * to that width; no result of the plan and none of its TEM state changes. */
int temxz_wave_create(temxz_wave** out, temx_plan* plan, const double* lon_deg_host /* [ncol] */, int nm,
                      const int* m_host /* [nm] */);
void temxz_wave_destroy(temxz_wave* wave);

/* device bytes the state holds now: the class tables, the weights and the workspace of the calls so far */
int64_t temxz_wave_workspace_bytes(const temxz_wave* wave);

/* The operator alone, for wavenumber m_host[mi]: Xc and Xs of nf in 1..TEMXZ_NF_MAX fields [ncol][D] (no theta
 * scaling), parts [nf][2][M][D], and on request the coefficients coef [nf][Kc][D].  TEMX_EINVAL: a null pointer, mi or
 * nf out of range, an unknown dtype, D outside [1, 2^28). */
int temxz_wave_project(temxz_wave* wave, int mi, int nf, const void* const* fields_host, const int* dtype_host,
                       int64_t D, double* parts, double* coef_or_null, void* stream);

/* The three wave-m fluxes of every wavenumber of the state, flux [nm][3][M][nlev][nt] in the order u'v', u'omega',
 * v'theta', and on request the parts of u, v, theta, omega, parts [nm][4][2][M][nlev][nt].  Needs temx_plan_set_tem
 * (TEMX_ESTATE otherwise); the fields are those of temx_tem_run; theta's column scale is applied as T is loaded.
 * TEMX_EUNSUPPORTED when the plan has been put into missing-value mode or on latitude bins since the state was made. */
int temxz_wave_fluxes(temxz_wave* wave, const void* ua, const void* va, const void* ta, const void* wap, int dtype,
                      double* flux, double* parts_or_null, void* stream);

/* Synchronises the stream and reports whether a non-finite value reached the sums of temxz_wave_project or
 * temxz_wave_fluxes since the last call, with a flag of the state's own.  Without this call a non-finite input goes
 * unreported: it comes out as NaN. */
int temxz_wave_status(temxz_wave* wave, int* nonfinite_host, void* stream);

/* How wavenumber m at truncation L (1 <= m <= L <= 511, TEMX_EINVAL otherwise; L + 1 - m > TEMXZ_NDEG_MAX:
 * TEMX_EUNSUPPORTED) is swept, as five ints: degrees L + 1 - m, Kc, blocks of four degrees per parity of l - m (TBS, the
 * instantiation), accumulators per field and lane (4 TBS), fields per wave.  Needs no device and no state. */
int temxz_wave_shape(int L, int m, int* shape_host);

/* How a sweep over D columns on wavenumber m_host[mi] is launched -- nf = 4: the four-field sweep of temxz_wave_fluxes,
 * nf = 1: the one-field sweep temxz_wave_project runs per field; any other nf is TEMX_EINVAL -- as four ints: TBS,
 * d-tiles of 16 columns, pieces of work the row table is cut into, and how many of the cuts between pieces fall inside a
 * class-group.  Host arithmetic only. */
int temxz_wave_launch(const temxz_wave* wave, int mi, int nf, int64_t D, int* out_host);

#ifdef __cplusplus
}
#endif

#endif /* TEMX_WAVECLS_H */
