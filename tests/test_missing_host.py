"""Missing-value mode (missing="mask"), host side: argument checks that must fail before any device call, the ABI
constants of include/temx.h, and the numpy MASKED ORACLE the GPU tests (test_gpu_missing.py) compare against, with
its self-checks.  Needs no GPU.

The oracle states the contract of include/temx.h ("Missing-value mode") directly:
  * per (level, time) column d: lstsq(w Y0, w a_filled), w = 1 on valid points and sqrt(tau) on missing ones,
    a_filled = 0 where missing -- every missing point an observation of 0 with weight tau;
  * common mask of u, v, T, omega; eddies NaN at missing points; products fitted the same way;
  * coverage = the factorised (default) operator applied to the validity indicator; the seven zonal means are NaN
    where coverage < min_coverage, then the epilogue of TEMOracle.from_zonal_means propagates NaN (np.gradient,
    cumulative trapezoid).
"""
import os
import re

import numpy as np
import pytest
import scipy.linalg

from oracle import tem_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROD = {"upvpb": ("up", "vp"), "upwappb": ("up", "wapp"), "vptpb": ("vp", "thetap")}


def masked_fit(Y0, fields, miss, tau):
    """Coefficients [nf][K][D] of the masked fits of fields [nf][N][D] under the mask miss [N][D]."""
    nf, N, D = fields.shape
    K = Y0.shape[1]
    C = np.empty((nf, K, D))
    sq = np.sqrt(tau)
    for d in range(D):
        m = miss[:, d]
        w = np.where(m, sq, 1.0)
        rhs = np.where(m[None, :], 0.0, fields[:, :, d]) * w[None, :]
        C[:, :, d] = scipy.linalg.lstsq(w[:, None] * Y0, rhs.T)[0].T
    return C


class MaskedOracle:
    """Masked TEM on ndarrays (ncol, lev, time), plev in hPa ascending (model top first)."""

    def __init__(self, ua, va, ta, wap, lat, plev, L, min_coverage=0.5, tau=1e-10, zm_dlat=1, p0=orc.P0):
        ua, va, ta, wap = (np.asarray(x, dtype=np.float64) for x in (ua, va, ta, wap))
        N, nlev, nt = ua.shape
        D = nlev * nt
        self.shape = (nlev, nt)
        self.plev = np.asarray(plev, dtype=np.float64)
        p = self.plev * 100
        theta = ta * ((p0 / p) ** orc.k)[None, :, None]
        self.lat_out = orc.zm_latitudes(zm_dlat)
        M = self.lat_out.size
        Y0 = orc.ylm0_matrix(lat, L)
        Y0p = orc.ylm0_matrix(self.lat_out, L)
        X = np.stack([x.reshape(N, D) for x in (ua, va, theta, wap)])
        self.miss = ~np.all(np.isfinite(X), axis=0)                       # common mask [N][D]
        C4 = masked_fit(Y0, X, self.miss, tau)
        eddy = X - np.einsum("ik,fkd->fid", Y0, C4)
        eddy[:, self.miss] = np.nan
        up, vp, thp, wp = eddy
        P = np.stack([up * vp, up * wp, vp * thp])
        C3 = masked_fit(Y0, P, self.miss, tau)
        za = orc.ZonalAverager(lat, self.lat_out, L, mode="factorised")
        valid = (~self.miss).astype(np.float64)
        self.coverage = za.zonal_mean(valid).reshape(M, nlev, nt)
        ccov = za.coefficients(valid)
        cov_native = Y0 @ ccov                                             # [N][D]
        thin_z = (self.coverage < min_coverage) if min_coverage > 0 else np.zeros_like(self.coverage, bool)
        thin_n = (cov_native < min_coverage) if min_coverage > 0 else np.zeros_like(cov_native, bool)
        zon = {}
        for i, n in enumerate(("ub", "vb", "thetab", "wapb")):
            zon[n] = (Y0p @ C4[i]).reshape(M, nlev, nt)
        for i, n in enumerate(("upvpb", "upwappb", "vptpb")):
            zon[n] = (Y0p @ C3[i]).reshape(M, nlev, nt)
        for n in zon:
            zon[n] = np.where(thin_z, np.nan, zon[n])
        tail = orc.TEMOracle.from_zonal_means(zon, self.plev, p0=p0, zm_dlat=zm_dlat)
        self.results = tail.results()
        self.zonal = tail.zonal_attrs()
        nat = {"up": up, "vp": vp, "thetap": thp, "wapp": wp, "upvp": P[0], "upwapp": P[1], "vptp": P[2]}
        self.native = {n: np.where(thin_n, np.nan, v).reshape(N, nlev, nt) for n, v in nat.items()}


def masked_zonal_mean(A, lat, lat_out, L, native=False, min_coverage=0.5, tau=1e-10):
    """The single-field operator in missing-value mode: A [N][D] -> [M][D] (or [N][D] when native)."""
    A = np.asarray(A, dtype=np.float64)
    miss = ~np.isfinite(A)
    Y0 = orc.ylm0_matrix(lat, L)
    C = masked_fit(Y0, A[None], miss, tau)[0]
    za = orc.ZonalAverager(lat, lat_out, L, mode="factorised")
    valid = (~miss).astype(np.float64)
    ccov = za.coefficients(valid)
    if native:
        out, cov = Y0 @ C, Y0 @ ccov
        out[miss] = np.nan
    else:
        out, cov = orc.ylm0_matrix(lat_out, L) @ C, za.zonal_mean(valid)
    if min_coverage > 0:
        out = np.where(cov < min_coverage, np.nan, out)
    return out, cov


def latlon(nlat, nlon):
    la = -90 + (np.arange(nlat) + 0.5) * 180.0 / nlat
    lo = np.arange(nlon) * 360.0 / nlon
    LA, LO = np.meshgrid(la, lo, indexing="ij")
    return LA.ravel().copy(), LO.ravel().copy()


def surface_mask(lat, lon, plev, nt):
    """Below-ground points of a synthetic surface pressure: a southern polar cap at 650 hPa, a plateau at 600 hPa,
    +-15 hPa of variation with time elsewhere.  True = missing, shape (ncol, nlev, nt)."""
    lat = np.asarray(lat)[:, None]
    lon = np.asarray(lon)[:, None]
    t = np.arange(nt)[None, :]
    ps = 1000.0 + 15.0 * np.sin(np.deg2rad(lon) + 0.7 * t) * np.cos(np.deg2rad(lat))
    ps = np.where(lat < -70.0, 650.0, ps)
    plateau = (np.abs(lat - 33.0) < 8.0) & (np.abs(lon - 88.0) < 15.0)
    ps = np.where(plateau, 600.0, ps)
    return np.asarray(plev)[None, :, None] > ps[:, None, :]


# ---- argument checks before any device call -----------------------------------------------------------------
def _tiny():
    lat, lon = latlon(6, 8)
    plev = np.array([100.0, 500.0, 1000.0])
    f = np.zeros((lat.size, 3, 1))
    return lat, plev, f


def test_temdiagnostics_rejects_unknown_missing_mode_before_device():
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match="missing"):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, missing="bogus")


def test_temdiagnostics_mask_with_tracer_not_implemented_before_device():
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(NotImplementedError, match="tracer"):
        TEMDiagnostics(f, f, f, f, lat, q=f, plev=plev, missing="mask")


def test_temdiagnostics_rejects_bad_min_coverage_before_device():
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match="min_coverage"):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, missing="mask", min_coverage=1.5)


def test_averager_rejects_unknown_missing_mode_before_device():
    from pytemdiags_amd import sph_zonal_averager
    lat, _, _ = _tiny()
    with pytest.raises(ValueError, match="missing"):
        sph_zonal_averager(lat, orc.zm_latitudes(1), 10, missing="nan")


def test_abi_constants_of_missing_mode():
    from pytemdiags_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "temx.h")).read()
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()

    def const(name):
        return int(re.search(r"\b%s\s*=\s*(-?\d+)" % name, hdr).group(1))
    assert const("TEMX_OPT_MISSING") == _lib.OPT_MISSING == 8
    assert const("TEMX_OPT_MIN_COVERAGE") == _lib.OPT_MIN_COVERAGE == 9
    assert const("TEMX_OPT_MISSING_WEIGHT") == _lib.OPT_MISSING_WEIGHT == 10
    assert const("TEMX_MAT_COVERAGE") == _lib.MAT_COVERAGE == 8
    assert const("TEMX_FORM_MASKED") == _lib.FORM_MASKED == 4
    assert _lib.ABI_VERSION == 402
    assert "int temx_version(void) { return 402; }" in src


# ---- self-checks of the masked oracle ------------------------------------------------------------------------
def test_masked_oracle_without_missing_points_is_the_default_pipeline():
    from pytemdiags_amd import synth
    lat, lon = latlon(24, 16)
    plev = synth.pressure_levels(8)
    ua, va, ta, wap = synth.analytic_fields(lat, lon, plev, 2, seed=5)
    mo = MaskedOracle(ua, va, ta, wap, lat, plev, 12)
    ref = orc.TEMOracle(ua, va, ta, wap, lat, plev, L=12, mode="factorised")
    assert np.all(mo.coverage > 0.999999)
    for n, r in ref.results().items():
        assert np.max(np.abs(mo.results[n] - r)) <= 1e-12 * np.max(np.abs(r)), n
    for n, r in ref.zonal_attrs().items():
        assert np.max(np.abs(mo.zonal[n] - r)) <= 1e-12 * max(np.max(np.abs(r)), 1e-300), n
    for n in ("up", "vp", "thetap", "wapp", "upvp", "upwapp", "vptp"):
        r = getattr(ref, n)
        assert np.max(np.abs(mo.native[n] - r)) <= 1e-12 * np.max(np.abs(r)), n


def test_masked_oracle_whole_missing_level_is_nan_and_other_levels_are_fitted():
    from pytemdiags_amd import synth
    lat, lon = latlon(24, 16)
    plev = synth.pressure_levels(8)
    ua, va, ta, wap = synth.analytic_fields(lat, lon, plev, 2, seed=6)
    lev = 7                                    # the lowest level: no data anywhere
    ta = ta.copy()
    ta[:, lev, :] = np.nan
    mo = MaskedOracle(ua, va, ta, wap, lat, plev, 12)
    ref = orc.TEMOracle(ua, va, np.nan_to_num(ta, nan=250.0), wap, lat, plev, L=12, mode="factorised")
    assert np.all(mo.coverage[:, lev, :] < 1e-6)
    for n in ("ub", "vb", "thetab", "wapb", "upvpb", "upwappb", "vptpb"):
        z = mo.zonal[n]
        assert np.all(np.isnan(z[:, lev, :])), n
        # the other levels are untouched by the empty one (their masks are empty)
        r = getattr(ref, n)
        assert np.max(np.abs(z[:, :lev, :] - r[:, :lev, :])) <= 1e-12 * np.max(np.abs(r[:, :lev, :])), n
    # the cumulative integral from the top never sees the empty level; the central difference in p does
    assert np.all(np.isfinite(mo.zonal["int_vbdp"][:, :lev, :]))
    assert np.all(np.isnan(mo.zonal["dub_dp"][:, lev - 1, :]))
    assert np.all(np.isfinite(mo.zonal["dub_dp"][:, : lev - 1, :]))


def test_masked_oracle_operator_and_surface_mask():
    from pytemdiags_amd import synth
    lat, lon = latlon(36, 24)
    plev = synth.pressure_levels(6)
    ua = synth.analytic_fields(lat, lon, plev, 2, seed=7)[0]
    miss = surface_mask(lat, lon, plev, 2)
    assert miss.any() and not miss.all()
    A = np.where(miss, np.nan, ua).reshape(lat.size, -1)
    lat_out = orc.zm_latitudes(3)
    z, cov = masked_zonal_mean(A, lat, lat_out, 15)
    # the polar cap below 650 hPa is empty: NaN there; the top levels are complete
    cap = lat_out < -75
    assert np.all(np.isnan(z.reshape(lat_out.size, 6, 2)[cap][:, -1]))
    top = orc.ZonalAverager(lat, lat_out, 15, mode="factorised").zonal_mean(ua.reshape(lat.size, -1))
    zt, tt = z.reshape(-1, 6, 2)[:, 0], top.reshape(-1, 6, 2)[:, 0]
    assert np.max(np.abs(zt - tt)) <= 1e-12 * np.max(np.abs(tt))
    zn, _ = masked_zonal_mean(A, lat, lat_out, 15, native=True)
    assert np.all(np.isnan(zn[np.isnan(A)]))
