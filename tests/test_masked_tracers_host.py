"""Tracer TEM for fields with missing values (missing="mask", tracer_mask="own"), host side: argument checks that must
fail before any device call, the sixth header (include/temx_mtracer.h) against its ctypes table and a plain-C consumer,
and the numpy MASKED TRACER ORACLE the GPU tests (test_gpu_masked_tracers.py) compare against, with its self-checks.
Needs no GPU.

The oracle states the contract of include/temx_mtracer.h directly, on top of MaskedOracle (test_missing_host.py):
  * the tracer's mask: q, v and omega all finite (u and T are not read);
  * qb: lstsq(w Y0, w q_filled) under that mask, w = 1 on valid points and sqrt(tau) on missing ones;
  * q' = q - qb(lat_i); v', omega' with the masked coefficients of the TEM run (its common mask); q'v', q'omega'
    fitted under the tracer's mask, 0 where the point is not valid;
  * tracer coverage = the factorised (default) operator applied to the tracer's validity indicator; qb, qpvpb,
    qpwappb NaN where it is below min_coverage; the rest by the tracer formulas of TEMOracle on the masked zonal
    means of the TEM run (NaN by propagation).
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import tem_oracle as orc
from test_missing_host import MaskedOracle, latlon, masked_fit, surface_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACER_ZONAL = ("qb", "qpvpb", "qpwappb", "dqb_dp", "qbcoslat", "dqbcoslat_dlat")
TRACER_NATIVE = ("qp", "qpvp", "qpwapp")


class MaskedTracerOracle:
    """One masked tracer on ndarrays (ncol, lev, time), plev in hPa ascending, next to the masked TEM run ``mo`` of
    the same ua, va, ta, wap (built here when not given)."""

    def __init__(self, ua, va, ta, wap, q, lat, plev, L, min_coverage=0.5, tau=1e-10, zm_dlat=1, p0=orc.P0, mo=None):
        va, wap, q = (np.asarray(x, dtype=np.float64) for x in (va, wap, q))
        self.mo = mo if mo is not None else MaskedOracle(ua, va, ta, wap, lat, plev, L, min_coverage=min_coverage,
                                                          tau=tau, zm_dlat=zm_dlat, p0=p0)
        mo = self.mo
        N, nlev, nt = q.shape
        D = nlev * nt
        M = mo.lat_out.size
        Y0 = orc.ylm0_matrix(lat, L)
        Y0p = orc.ylm0_matrix(mo.lat_out, L)
        V = np.stack([va.reshape(N, D), wap.reshape(N, D)])
        Q = q.reshape(N, D)
        # v', omega': the eddies of the TEM run (its common mask)
        Cvw = masked_fit(Y0, V, mo.miss, tau)
        self.miss = ~(np.isfinite(Q) & np.all(np.isfinite(V), axis=0))       # the tracer's own mask [N][D]
        Cq = masked_fit(Y0, Q[None], self.miss, tau)[0]
        qp = Q - Y0 @ Cq
        vp, wp = V - np.einsum("ik,fkd->fid", Y0, Cvw)
        qp[self.miss] = np.nan
        P = np.stack([qp * vp, qp * wp])
        P[:, self.miss] = np.nan
        C2 = masked_fit(Y0, P, self.miss, tau)
        za = orc.ZonalAverager(lat, mo.lat_out, L, mode="factorised")
        valid = (~self.miss).astype(np.float64)
        self.coverage = za.zonal_mean(valid).reshape(M, nlev, nt)
        cov_native = Y0 @ za.coefficients(valid)
        thin_z = (self.coverage < min_coverage) if min_coverage > 0 else np.zeros_like(self.coverage, bool)
        thin_n = (cov_native < min_coverage) if min_coverage > 0 else np.zeros_like(cov_native, bool)
        zon = {"qb": Y0p @ Cq, "qpvpb": Y0p @ C2[0], "qpwappb": Y0p @ C2[1]}
        zon = {n: np.where(thin_z, np.nan, z.reshape(M, nlev, nt)) for n, z in zon.items()}
        tail = orc.TEMOracle.from_zonal_means({n: mo.zonal[n] for n in ("ub", "vb", "thetab", "wapb", "upvpb",
                                                                         "upwappb", "vptpb")},
                                              mo.plev, p0=p0, zm_dlat=zm_dlat)
        tail.qb, tail.qpvpb, tail.qpwappb = [zon["qb"]], [zon["qpvpb"]], [zon["qpwappb"]]
        tail.q = [np.empty(0, dtype=np.float64)]
        tail._derivatives()
        self.results = tail.tracer_results(0)
        self.zonal = dict(zon, dqb_dp=tail.dqb_dp[0], qbcoslat=tail.qbcoslat[0], dqbcoslat_dlat=tail.dqbcoslat_dlat[0])
        nat = {"qp": qp, "qpvp": P[0], "qpwapp": P[1]}
        self.native = {n: np.where(thin_n, np.nan, v).reshape(N, nlev, nt) for n, v in nat.items()}


def tracer_gap(lat, lon, plev, nt):
    """A gap only the tracer has: -20 < lat < 10, 100 < lon < 320, below 300 hPa.  True = missing, (ncol, nlev, nt)."""
    lat, lon = np.asarray(lat), np.asarray(lon)
    cols = (lat > -20.0) & (lat < 10.0) & (lon > 100.0) & (lon < 320.0)
    return np.broadcast_to(cols[:, None, None] & (np.asarray(plev) > 300.0)[None, :, None], (lat.size, len(plev), nt)).copy()


def masked_tracer_fields(lat, lon, nlev, nt, dtype=np.float64, gap=True, which=0):
    """ua, va, ta, wap, q of ``synth.analytic_fields(seed=1)`` / ``synth.analytic_tracer`` on the levels of
    test_gpu_missing.masked_fields, NaN below the synthetic surface in all five and, with ``gap``, in ``tracer_gap``
    in the tracer alone.  -> (plev, [ua, va, ta, wap], q)"""
    from pytemdiags_amd import synth
    plev = np.sort(synth.pressure_levels(nlev) * 0.5 + 500.0 * np.linspace(0, 1, nlev) ** 2)
    f = list(synth.analytic_fields(lat, lon, plev, nt, seed=1)) + [synth.analytic_tracer(lat, lon, plev, nt, which=which)]
    miss = surface_mask(lat, lon, plev, nt)
    f = [np.where(miss, np.nan, x).astype(dtype) for x in f]
    if gap:
        f[4] = np.where(tracer_gap(lat, lon, plev, nt), np.nan, f[4]).astype(dtype)
    return plev, f[:4], f[4]


# ---- self-checks of the masked tracer oracle -------------------------------------------------------------------
def test_masked_tracer_oracle_without_missing_points_is_the_default_tracer_pipeline():
    from pytemdiags_amd import synth
    lat, lon = latlon(24, 16)
    plev = synth.pressure_levels(8)
    f = synth.analytic_fields(lat, lon, plev, 2, seed=5)
    q = synth.analytic_tracer(lat, lon, plev, 2)
    to = MaskedTracerOracle(*f, q, lat, plev, 12)
    ref = orc.TEMOracle(*f, lat, plev, L=12, mode="factorised", q=q)
    assert np.all(to.coverage > 0.999999)
    worst = 0.0
    for n, r in ref.tracer_results(0).items():
        worst = max(worst, float(np.max(np.abs(to.results[n] - r)) / np.max(np.abs(r))))
    for n in TRACER_ZONAL:
        r = getattr(ref, n)[0]
        worst = max(worst, float(np.max(np.abs(to.zonal[n] - r)) / np.max(np.abs(r))))
    for n in TRACER_NATIVE:
        r = getattr(ref, n)[0]
        worst = max(worst, float(np.max(np.abs(to.native[n] - r)) / np.max(np.abs(r))))
    print("masked tracer oracle against the default pipeline, worst field-normalised difference %.2e" % worst)
    assert worst <= 1e-12


def test_masked_tracer_oracle_tracer_gap_thins_the_tracer_only():
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(8)
    plev, f, q = masked_tracer_fields(lat, lon, 7, 3)
    to = MaskedTracerOracle(*f, q, lat, plev, 20)
    assert np.array_equal(to.mo.miss, ~np.all(np.isfinite(np.stack([x.reshape(lat.size, -1) for x in f])), axis=0))
    assert np.all(to.miss[to.mo.miss]) and to.miss.sum() > to.mo.miss.sum()        # the gap is the tracer's alone
    assert np.any(to.coverage < to.mo.coverage - 0.05)
    thin_t, thin_m = float(np.mean(to.coverage < 0.5)), float(np.mean(to.mo.coverage < 0.5))
    print("thin share of the zonal grid: tracer %.3f, TEM run %.3f" % (thin_t, thin_m))
    assert thin_t > thin_m > 0.0
    # the tracer's NaN reach the results by propagation, the TEM run's results are not touched
    assert np.isnan(to.zonal["qb"]).sum() > np.isnan(to.mo.zonal["ub"]).sum()
    assert np.array_equal(np.isnan(to.native["qp"]), np.isnan(to.native["qpvp"]))
    assert np.all(np.isnan(to.native["qp"])[to.miss.reshape(to.native["qp"].shape)])


# ---- argument checks before any device call --------------------------------------------------------------------
def _tiny():
    lat, lon = latlon(6, 8)
    plev = np.array([100.0, 500.0, 1000.0])
    return lat, plev, np.zeros((lat.size, 3, 1))


def test_temdiagnostics_tracer_mask_checks_before_device():
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match="tracer_mask"):
        TEMDiagnostics(f, f, f, f, lat, q=f, plev=plev, missing="mask", tracer_mask="bogus")
    with pytest.raises(ValueError, match="tracer_mask"):
        TEMDiagnostics(f, f, f, f, lat, q=f, plev=plev, missing="raise", tracer_mask="own")
    with pytest.raises(ValueError, match="tracer_mask"):
        TEMDiagnostics(f, f, f, f, lat, q=f, plev=plev, tracer_mask="own")
    with pytest.raises(NotImplementedError, match="tracer_mask"):
        TEMDiagnostics(f, f, f, f, lat, q=f, plev=plev, missing="mask")


def test_from_model_levels_tracer_mask_checks_before_device():
    from pytemdiags_amd import TEMDiagnostics
    lat = np.linspace(-80, 80, 5)
    f = np.zeros((5, 8, 2))
    eta = np.linspace(0.01, 0.99, 8)
    kw = dict(plev=[500.0], ps=np.full((5, 2), 1e5), hyam=eta * 0.1, hybm=eta * 0.9, q=f)
    with pytest.raises(ValueError, match="tracer_mask"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, missing="mask", tracer_mask="bogus", **kw)
    with pytest.raises(ValueError, match="tracer_mask"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, missing="raise", tracer_mask="own", **kw)
    with pytest.raises(NotImplementedError, match="tracer_mask"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, missing="mask", **kw)


# ---- header, bindings, plain-C consumer ------------------------------------------------------------------------
def test_mtracer_header_declares_exactly_what_is_bound():
    import ctypes as C
    from pytemdiags_amd import _lib, _mtracer
    hdr = open(os.path.join(ROOT, "include", "temx_mtracer.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(temxm_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _mtracer.SIGNATURES} == {"temxm_version", "temxm_tracer_run", "temxm_tracer_eddy"}
    assert not re.findall(r"\b(temx[vlic]?_[a-z0-9_]+)\s*\(", code)     # the other headers' ABI is not extended from here
    lib = _mtracer.load()
    assert lib is _lib.load() and lib.temxm_version() == _mtracer.MTRACER_VERSION == 100
    ctype = {"int": C.c_int, "void*": C.c_void_p, "const void*": C.c_void_p, "double*": C.c_void_p,
             "temx_plan*": C.c_void_p, "double* const*": C.POINTER(C.c_void_p)}
    sig = dict((n, (r, a)) for n, r, a in _mtracer.SIGNATURES)
    names = {}
    for fn in ("temxm_tracer_run", "temxm_tracer_eddy"):
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert sig[fn] == (C.c_int, [ctype[p.rsplit(" ", 1)[0]] for p in params]), fn
        names[fn] = [p.rsplit(" ", 1)[1] for p in params]
    assert sig["temxm_version"] == (C.c_int, [])
    assert names["temxm_tracer_run"] == ["plan", "q", "va", "wap", "dtype", "tres", "tzon_or_null", "tcov_or_null", "stream"]
    assert names["temxm_tracer_eddy"] == ["plan", "q", "va", "wap", "dtype", "ptrs3_host", "stream"]
    # function-try-blocks like every other entry point; the first header gains no function and keeps its version
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    for fn in ("temxm_tracer_run", "temxm_tracer_eddy"):
        assert re.search(r"^int %s\([^;{]*\)\s*try \{\s*$" % fn, src, re.M), fn
    assert "int temx_version(void) { return 402; }" in src and "int temxm_version(void) { return 100; }" in src
    first = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "temx.h")).read(), flags=re.S)
    assert "temxm_" not in first and _lib.ABI_VERSION == 402


def test_mtracer_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_mtracer")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_mtracer.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxm_version=100 null_plan_run_rc=-1 null_plan_eddy_rc=-1" in out.stdout
    assert "temx_version=402" in out.stdout


def test_mtracer_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _mtracer
    lib = _mtracer.load()
    p = C.c_void_p(4096)
    ptrs = (C.c_void_p * 3)(4096, 4096, 4096)
    assert lib.temxm_tracer_run(None, p, p, p, 0, p, None, None, None) == -1
    assert lib.temxm_tracer_eddy(None, p, p, p, 0, ptrs, None) == -1
    assert b"null" in lib.temx_last_error()
