"""Missing-value mode on the MI355X: the masked TEM pipeline, the masked operator and the front end against the
numpy masked oracle of test_missing_host.py; NaN-free input against the default path; level independence; edge
cases (an empty level, min_coverage = 0, the default still raising, unsupported entry points, repeatability)."""
import numpy as np
import pytest

from oracle import tem_oracle as orc
from test_missing_host import MaskedOracle, latlon, masked_zonal_mean, surface_mask

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RESULTS = ("vtem", "omegatem", "wtem", "psitem", "epfy", "epfz", "epdiv", "utendepfd", "utendvtem", "utendwtem")
ZONAL = ("ub", "vb", "thetab", "wapb", "upvpb", "upwappb", "vptpb", "dub_dp", "dthetab_dp", "ubcoslat",
         "dubcoslat_dlat", "psi", "psicoslat", "dpsicoslat_dlat", "dpsi_dp", "int_vbdp")
NATIVE = ("up", "vp", "thetap", "wapp", "upvp", "upwapp", "vptp")
THR = 0.5
# fp64 bound of the masked fit at high degree with an empty polar cap.  The per-column normal equations of the masked
# fit have a condition number up to ~1/tau (1e10): measured 2.7e-7 (cubed sphere, L = 50) and 1.7e-5 (2-degree lat-lon
# grid, L = 63) against the oracle's lstsq on the weighted rows; 1e-12 at L = 20 (missing-value mode).
CAP_TOL = {50: 1e-6, 63: 5e-5}


def tol_of(L, dtype):
    return max(1e-9 if dtype == np.float64 else 2e-5, CAP_TOL.get(L, 0.0))


def grid(kind):
    from pytemdiags_amd import synth
    if kind == "cs8":
        return synth.cubed_sphere_gll(8)
    if kind == "latlon2":
        return latlon(90, 180)
    rng = np.random.default_rng(3)                   # unstructured: random latitudes and longitudes
    n = 3000
    return np.rad2deg(np.arcsin(rng.uniform(-1, 1, n))), rng.uniform(0, 360, n)


def masked_fields(kind, nlev=8, nt=2, seed=1, dtype=np.float64):
    from pytemdiags_amd import synth
    lat, lon = grid(kind)
    plev = synth.pressure_levels(nlev) * 0.5 + 500.0 * np.linspace(0, 1, nlev) ** 2   # dense near the surface
    plev = np.sort(plev)
    f = [x.astype(dtype) for x in synth.analytic_fields(lat, lon, plev, nt, seed=seed)]
    miss = surface_mask(lat, lon, plev, nt)
    f = [np.where(miss, np.nan, x).astype(dtype) for x in f]
    return lat, lon, plev, f, miss


def err(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref) & np.isfinite(x)
    den = np.max(np.abs(ref[fin])) if fin.any() else 0.0
    return float(np.max(np.abs(x[fin] - ref[fin])) / den) if den > 0 else float(np.max(np.abs(x[fin]), initial=0.0))


def ambiguous(cov):
    """(lat, time) columns of the zonal grid whose coverage lies within 1e-9 of the threshold somewhere, widened by
    one latitude (the stencils reach there): their NaN pattern may legitimately differ."""
    a = np.any(np.abs(cov - THR) < 1e-9, axis=1)                  # [M][nt]
    a = a | np.roll(a, 1, axis=0) | np.roll(a, -1, axis=0)
    return a[:, None, :]


def same_nans(x, ref, amb):
    x, ref = np.asarray(x), np.asarray(ref)
    diff = (np.isnan(x) != np.isnan(ref)) & ~np.broadcast_to(amb, ref.shape)
    return int(np.count_nonzero(diff))


def run_plan(lat, plev, f, L, mask=True, min_coverage=THR, **kw):
    from pytemdiags_amd import engine
    nlev, nt = f[0].shape[1:]
    plan = engine.Plan(lat, orc.zm_latitudes(1), L, device=0, fp32_fields=f[0].dtype == np.float32, **kw)
    if mask:
        plan.configure(missing="mask", min_coverage=min_coverage)
    plan.set_tem(nlev, nt, plev * 100)
    dev = [torch.as_tensor(x, device="cuda:0") for x in f]
    res, zon = plan.tem_run(*dev, want_zonal=True)
    M = plan.M
    out = {"res": res.cpu().numpy().reshape(10, M, nlev, nt), "zon": zon.cpu().numpy().reshape(16, M, nlev, nt)}
    if mask:
        out["cov"] = plan.coverage().cpu().numpy().reshape(M, nlev, nt)
    return plan, dev, out


@pytest.mark.parametrize("kind,L,dtype", [("cs8", 50, np.float64), ("latlon2", 63, np.float32),
                                          ("random", 20, np.float64), ("cs8", 63, np.float32)])
def test_masked_tem_matches_masked_oracle(kind, L, dtype):
    lat, lon, plev, f, miss = masked_fields(kind, dtype=dtype)
    tol = tol_of(L, dtype)
    plan, dev, out = run_plan(lat, plev, f, L)
    assert plan.option(8) == 1 and plan.option(1) == 4        # TEMX_OPT_MISSING, TEMX_FORM_MASKED
    assert not plan.status()                                   # non-finite input is data in this mode
    mo = MaskedOracle(*f, lat, plev, L, min_coverage=THR)
    amb = ambiguous(mo.coverage)
    assert err(out["cov"], mo.coverage) <= tol
    for i, n in enumerate(RESULTS):
        assert err(out["res"][i], mo.results[n]) <= tol, (n, err(out["res"][i], mo.results[n]))
        assert same_nans(out["res"][i], mo.results[n], amb) == 0, n
    for i, n in enumerate(ZONAL):
        assert err(out["zon"][i], mo.zonal[n]) <= tol, (n, err(out["zon"][i], mo.zonal[n]))
        assert same_nans(out["zon"][i], mo.zonal[n], amb) == 0, n
    assert np.isnan(out["zon"][0]).any() and np.isfinite(out["zon"][0]).any()
    # native eddy fields: whole and by rows
    eddy = plan.tem_eddy(*dev)
    for n in NATIVE:
        e = eddy[n].cpu().numpy()
        assert err(e, mo.native[n]) <= tol, (n, err(e, mo.native[n]))
        assert np.array_equal(np.isnan(e), np.isnan(mo.native[n])), n
    rows = plan.tem_eddy_rows(*dev, 16, 64)
    for n in NATIVE:
        assert np.array_equal(rows[n].cpu().numpy(), eddy[n].cpu().numpy()[16:80], equal_nan=True), n


@pytest.mark.parametrize("kind,L,dtype", [("cs8", 50, np.float64), ("latlon2", 20, np.float32), ("random", 63, np.float64)])
def test_masked_operator_matches_masked_oracle(kind, L, dtype):
    from pytemdiags_amd import sph_zonal_averager
    lat, lon, plev, f, miss = masked_fields(kind, dtype=dtype)
    tol = tol_of(L, dtype)
    lat_out = orc.zm_latitudes(1)
    za = sph_zonal_averager(lat, lat_out, L, missing="mask")
    za.sph_compute_matrices()
    A = f[0]
    z = za.sph_zonal_mean(A)
    zn = za.sph_zonal_mean_native(A)
    assert z.dtype == A.dtype and zn.dtype == A.dtype and z.shape == (lat_out.size,) + A.shape[1:]
    ref, cov = masked_zonal_mean(A.reshape(A.shape[0], -1), lat, lat_out, L)
    refn, _ = masked_zonal_mean(A.reshape(A.shape[0], -1), lat, lat_out, L, native=True)
    ref, refn = ref.reshape(z.shape), refn.reshape(zn.shape)
    amb = ambiguous(cov.reshape(z.shape))
    assert err(z, ref) <= tol and same_nans(z, ref, amb) == 0
    assert err(zn, refn) <= tol
    assert np.array_equal(np.isnan(zn), np.isnan(refn))
    assert err(za._plan.coverage().cpu().numpy().reshape(z.shape), cov.reshape(z.shape)) <= tol


def test_nan_free_input_equals_default_path():
    from pytemdiags_amd import synth
    for kind, form in (("cs8", "single-sweep"), ("random", None)):
        lat, lon = grid(kind)
        nlev, nt = 16, 4                                         # D = 64: four d-tiles, the single sweep's minimum
        plev = synth.pressure_levels(nlev)
        f = synth.analytic_fields(lat, lon, plev, nt, seed=4)
        plan, dev, ref = run_plan(lat, plev, f, 50, mask=False, form=form)
        if form == "single-sweep":
            assert plan.single_sweep
        plan.configure(missing="mask")
        plan.set_tem(nlev, nt, plev * 100)
        res, zon = plan.tem_run(*dev, want_zonal=True)
        res, zon = res.cpu().numpy().reshape(ref["res"].shape), zon.cpu().numpy().reshape(ref["zon"].shape)
        for i, n in enumerate(RESULTS):
            assert err(res[i], ref["res"][i]) <= 1e-11, (kind, n, err(res[i], ref["res"][i]))
        for i, n in enumerate(ZONAL):
            assert err(zon[i], ref["zon"][i]) <= 1e-11, (kind, n, err(zon[i], ref["zon"][i]))
        assert np.all(np.isfinite(res)) and np.all(np.isfinite(zon))
        assert np.max(np.abs(plan.coverage().cpu().numpy() - 1.0)) <= 1e-11


def test_levels_without_missing_points_equal_default_on_filled_copy():
    lat, lon, plev, f, miss = masked_fields("cs8", nlev=10, nt=3)
    _, _, out = run_plan(lat, plev, f, 40)
    filled = [np.where(miss, 123.0 + 7.0 * i, x) for i, x in enumerate(f)]
    _, _, ref = run_plan(lat, plev, filled, 40, mask=False)
    clean = ~miss.any(axis=0)                                   # [nlev][nt]: d with no missing point
    assert clean.any() and not clean.all()
    for i in range(7):
        a, b = out["zon"][i][:, clean], ref["zon"][i][:, clean]
        assert err(a, b) <= 1e-11, (ZONAL[i], err(a, b))


def test_empty_level_is_nan_and_min_coverage_zero():
    from pytemdiags_amd import synth
    lat, lon = grid("latlon2")
    plev = synth.pressure_levels(8)
    f = list(synth.analytic_fields(lat, lon, plev, 2, seed=9))
    filled = [x.copy() for x in f]
    f[1] = f[1].copy()
    f[1][:, 7, :] = np.nan
    _, _, out = run_plan(lat, plev, f, 30)
    _, _, ref = run_plan(lat, plev, filled, 30, mask=False)
    for i in range(7):
        assert np.all(np.isnan(out["zon"][i][:, 7, :])), ZONAL[i]
        assert err(out["zon"][i][:, :7], ref["zon"][i][:, :7]) <= 1e-11, ZONAL[i]
    # min_coverage = 0: no coverage NaN, the empty polar cap is fitted (weakly) like everything else
    lat, lon, plev, g, miss = masked_fields("cs8")
    _, _, out0 = run_plan(lat, plev, g, 30, min_coverage=0.0)
    for i in range(7):
        assert np.all(np.isfinite(out0["zon"][i])), ZONAL[i]


def test_default_mode_still_raises_on_nan():
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, miss = masked_fields("cs8", nlev=6, nt=1)
    with pytest.raises(RuntimeError, match="nans"):
        TEMDiagnostics(*f, lat, plev=plev, L=20, debug_level=0)


def test_frontend_masked_and_coverage():
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, miss = masked_fields("cs8", nlev=8, nt=2)
    tem = TEMDiagnostics(*f, lat, plev=plev, L=30, debug_level=0, missing="mask")
    mo = MaskedOracle(*f, lat, plev, 30)
    amb = ambiguous(mo.coverage)
    assert err(np.asarray(tem.coverage), mo.coverage) <= 1e-9
    for n in RESULTS:
        x = np.asarray(getattr(tem, n)())
        assert err(x, mo.results[n]) <= 1e-9 and same_nans(x, mo.results[n], amb) == 0, n
    for n in ("ub", "vptpb", "int_vbdp"):
        assert err(np.asarray(getattr(tem, n)), mo.zonal[n]) <= 1e-9, n
    assert err(np.asarray(tem.upvp), mo.native["upvp"]) <= 1e-9
    for c0, c1, blk in tem.iter_native(names=("vp",), chunk_cols=1024):
        assert np.array_equal(blk["vp"], np.asarray(tem.vp)[c0:c1], equal_nan=True)


def test_unsupported_in_masked_mode():
    from pytemdiags_amd import _lib, engine, synth
    lat, lon = grid("cs8")
    plev = synth.pressure_levels(6)
    f = [torch.as_tensor(x, device="cuda:0") for x in synth.analytic_fields(lat, lon, plev, 2, seed=2)]
    plan = engine.Plan(lat, orc.zm_latitudes(1), 20, device=0)
    plan.configure(missing="mask")
    plan.set_tem(6, 2, plev * 100)
    calls = [lambda: plan.tem_stage1(*f), lambda: plan.project(f[0]), lambda: plan.tracer_run(f[0], f[1], f[3]),
             lambda: plan.tem_os_prepass(*f)]
    for c in calls:
        with pytest.raises(_lib.TemxError) as ei:
            c()
        assert ei.value.code == -6
    big = engine.Plan(lat, orc.zm_latitudes(1), 64, device=0)
    with pytest.raises(_lib.TemxError) as ei:
        big.configure(missing="mask")
    assert ei.value.code == -6
    w = engine.Plan(lat, orc.zm_latitudes(1), 20, device=0, defer_finalize=True)
    w.set_weights(np.full(lat.size, 1.0 / lat.size))
    with pytest.raises(_lib.TemxError) as ei:
        w.configure(missing="mask")
    assert ei.value.code == -6
    fresh = engine.Plan(lat, orc.zm_latitudes(1), 20, device=0)
    with pytest.raises(_lib.TemxError) as ei:
        fresh.matrix_cov = fresh.coverage()
    assert ei.value.code == -5
    from pytemdiags_amd.sharding import NcolShardedTEM
    with pytest.raises(NotImplementedError):
        NcolShardedTEM(plan)


def test_repeated_masked_runs_are_bitwise_identical():
    lat, lon, plev, f, miss = masked_fields("random", nlev=6, nt=2)
    plan, dev, a = run_plan(lat, plev, f, 50)
    res, zon = plan.tem_run(*dev, want_zonal=True)
    assert np.array_equal(res.cpu().numpy().reshape(a["res"].shape), a["res"], equal_nan=True)
    assert np.array_equal(zon.cpu().numpy().reshape(a["zon"].shape), a["zon"], equal_nan=True)
