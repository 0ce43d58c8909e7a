"""Tracer TEM for fields with missing values on the MI355X (include/temx_mtracer.h; missing="mask", tracer_mask="own"):
the masked tracer run, its native fields and the front end against the numpy masked tracer oracle of
test_masked_tracers_host.py; NaN-free input against the default tracer path; a tracer missing exactly where the fields
are; an empty level and min_coverage = 0; state and errors; repeatability and isolation of the plan's TEM state.

Shapes: the smallest at which the tiling can go wrong.  cs8 has N = 3458 = 216 * 16 + 2 columns (a ragged last chunk);
L = 50 on 7 x 3 gives D = 21 (a ragged d-tile and idle waves in the quad) and K = 51 (no multiple of 4); L = 63 on
8 x 2 gives K = 64 and D = 16; the unstructured grid has 3000 columns.
Bounds: ``tol_of`` of test_gpu_missing.py for the comparison with the oracle (the masked fit's conditioning, derived
there); 1e-11 where two GPU paths compute the same fit; 1e-9 for the front end, as test_frontend_masked_and_coverage.
Measured against the oracle (worst of coverage, results, zonal and native fields): 2.9e-7 at L = 50 fp64 (bound 1e-6),
1.7e-12 at L = 20 fp64 (1e-9), 1.5e-7 at L = 63 fp32 (5e-5); no ambiguous (lat, time) column in any case."""
import numpy as np
import pytest

from oracle import tem_oracle as orc
from test_gpu_missing import THR, ambiguous, err, grid, same_nans, tol_of
from test_masked_tracers_host import (TRACER_NATIVE, TRACER_ZONAL, MaskedTracerOracle, masked_tracer_fields,
                                      tracer_gap)
from test_missing_host import MaskedOracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRACER_RESULTS = ("etfy", "etfz", "etdiv", "qtendetfd", "qtendvtem", "qtendwtem")
CASES = [("cs8", 50, 7, 3, np.float64), ("random", 20, 7, 3, np.float64), ("cs8", 63, 8, 2, np.float32)]
_cache = {}


def case(kind, L, nlev, nt, dtype):
    """Inputs and oracle of one shape, computed once and left unchanged."""
    key = (kind, L, nlev, nt, np.dtype(dtype).name)
    if key not in _cache:
        lat, lon = grid(kind)
        plev, f, q = masked_tracer_fields(lat, lon, nlev, nt, dtype=dtype)
        _cache[key] = (lat, lon, plev, f, q, MaskedTracerOracle(*f, q, lat, plev, L, min_coverage=THR))
    return _cache[key]


def masked_plan(lat, plev, f, L, mask=True, min_coverage=THR, **kw):
    """A plan after ``tem_run`` on ``f`` (in missing-value mode unless ``mask`` is False) and the device fields."""
    from pytemdiags_amd import engine
    nlev, nt = f[0].shape[1:]
    plan = engine.Plan(lat, orc.zm_latitudes(1), L, device=0, fp32_fields=f[0].dtype == np.float32, **kw)
    if mask:
        plan.configure(missing="mask", min_coverage=min_coverage)
    plan.set_tem(nlev, nt, plev * 100)
    dev = [torch.as_tensor(x, device="cuda:0") for x in f]
    plan.tem_run(*dev)
    return plan, dev


def tracer_out(plan, dev, q):
    qd = torch.as_tensor(q, device="cuda:0")
    tres, tzon, tcov = plan.tracer_run_masked(qd, dev[1], dev[3], want_zonal=True)
    return qd, tres.cpu().numpy(), tzon.cpu().numpy(), tcov.cpu().numpy()


@pytest.mark.parametrize("kind,L,nlev,nt,dtype", CASES)
def test_masked_tracer_run_and_native_fields_match_the_oracle(kind, L, nlev, nt, dtype):
    lat, lon, plev, f, q, to = case(kind, L, nlev, nt, dtype)
    tol = tol_of(L, dtype)
    plan, dev = masked_plan(lat, plev, f, L)
    qd, tres, tzon, tcov = tracer_out(plan, dev, q)
    assert not plan.status()                                   # non-finite input is data in this mode
    amb = ambiguous(to.coverage) | ambiguous(to.mo.coverage)
    assert float(np.mean(amb)) <= 0.01
    e = err(tcov, to.coverage)
    print("%s L=%d %s: coverage %.2e" % (kind, L, np.dtype(dtype).name, e))
    assert e <= tol
    for i, n in enumerate(TRACER_RESULTS):
        e = err(tres[i], to.results[n])
        print("  %-14s %.2e (tol %.1e)" % (n, e, tol))
        assert e <= tol, (n, e)
        assert same_nans(tres[i], to.results[n], amb) == 0, n
    for i, n in enumerate(TRACER_ZONAL):
        e = err(tzon[i], to.zonal[n])
        print("  %-14s %.2e (tol %.1e)" % (n, e, tol))
        assert e <= tol, (n, e)
        assert same_nans(tzon[i], to.zonal[n], amb) == 0, n
    assert np.isnan(tzon[0]).any() and np.isfinite(tzon[0]).any()
    # the tracer's gap costs coverage the TEM run keeps
    assert np.any(tcov < plan.coverage().cpu().numpy().reshape(tcov.shape) - 0.05)
    # native fields: values within the tolerance, the NaN pattern exactly the oracle's
    eddy = plan.tracer_eddy_masked(qd, dev[1], dev[3])
    for n in TRACER_NATIVE:
        x = eddy[n].cpu().numpy()
        e = err(x, to.native[n])
        print("  %-14s %.2e (tol %.1e)" % (n, e, tol))
        assert e <= tol, (n, e)
        assert np.array_equal(np.isnan(x), np.isnan(to.native[n])), n


def test_nan_free_input_equals_default_tracer_path():
    from pytemdiags_amd import synth
    for kind, form in (("cs8", "single-sweep"), ("random", None)):
        lat, lon = grid(kind)
        nlev, nt = 16, 4                                         # D = 64: four d-tiles, the single sweep's minimum
        plev = synth.pressure_levels(nlev)
        f = synth.analytic_fields(lat, lon, plev, nt, seed=4)
        q = synth.analytic_tracer(lat, lon, plev, nt)
        plan, dev = masked_plan(lat, plev, f, 50, mask=False, form=form)
        qd = torch.as_tensor(q, device="cuda:0")
        rres, rzon = (x.cpu().numpy() for x in plan.tracer_run(qd, dev[1], dev[3], want_zonal=True))
        plan.configure(missing="mask")
        plan.set_tem(nlev, nt, plev * 100)
        plan.tem_run(*dev)
        tres, tzon, tcov = (x.cpu().numpy() for x in plan.tracer_run_masked(qd, dev[1], dev[3], want_zonal=True))
        for i, n in enumerate(TRACER_RESULTS):
            assert err(tres[i], rres[i]) <= 1e-11, (kind, n, err(tres[i], rres[i]))
        for i, n in enumerate(TRACER_ZONAL):
            assert err(tzon[i], rzon[i]) <= 1e-11, (kind, n, err(tzon[i], rzon[i]))
        assert np.all(np.isfinite(tres)) and np.all(np.isfinite(tzon))
        assert np.max(np.abs(tcov - 1.0)) <= 1e-11


def test_tracer_missing_where_the_fields_are_has_the_coverage_of_the_tem_run():
    lat, lon = grid("cs8")
    plev, f, q = masked_tracer_fields(lat, lon, 7, 3, gap=False)
    plan, dev = masked_plan(lat, plev, f, 50)
    _, tres, tzon, tcov = tracer_out(plan, dev, q)
    cov = plan.coverage().cpu().numpy().reshape(tcov.shape)
    assert np.max(np.abs(tcov - cov)) <= 1e-11
    assert np.isnan(tzon[0]).any() and np.isfinite(tzon[0]).any()


def test_empty_tracer_level_is_nan_and_min_coverage_zero():
    from pytemdiags_amd import synth
    lat, lon = grid("latlon2")
    plev = synth.pressure_levels(8)
    f = list(synth.analytic_fields(lat, lon, plev, 2, seed=9))
    filled = synth.analytic_tracer(lat, lon, plev, 2)
    q = filled.copy()
    q[:, 7, :] = np.nan
    plan, dev = masked_plan(lat, plev, f, 30)
    _, tres, tzon, tcov = tracer_out(plan, dev, q)
    _, rres, rzon, rcov = tracer_out(plan, dev, filled)
    for i in range(3):
        assert np.all(np.isnan(tzon[i][:, 7, :])), TRACER_ZONAL[i]
        assert err(tzon[i][:, :7], rzon[i][:, :7]) <= 1e-11, TRACER_ZONAL[i]
    assert np.max(np.abs(tcov[:, 7, :])) <= 1e-6 and np.max(np.abs(tcov[:, :7] - 1.0)) <= 1e-11
    # min_coverage = 0: no coverage NaN, the tracer's gap and the empty polar cap are fitted (weakly) like the rest
    lat, lon, plev, g, q, _ = case("cs8", 50, 7, 3, np.float64)
    plan0, dev0 = masked_plan(lat, plev, g, 30, min_coverage=0.0)
    _, _, tzon0, _ = tracer_out(plan0, dev0, q)
    for i in range(3):
        assert np.all(np.isfinite(tzon0[i])), TRACER_ZONAL[i]


def test_state_and_errors():
    from pytemdiags_amd import _lib, engine
    lat, lon, plev, f, q, _ = case("random", 20, 7, 3, np.float64)
    dev = [torch.as_tensor(x, device="cuda:0") for x in f]
    qd = torch.as_tensor(q, device="cuda:0")

    def code_of(call):
        with pytest.raises(_lib.TemxError) as ei:
            call()
        return ei.value.code
    plan = engine.Plan(lat, orc.zm_latitudes(1), 20, device=0)
    plan.configure(missing="mask")
    plan.set_tem(7, 3, plev * 100)
    assert code_of(lambda: plan.tracer_run_masked(qd, dev[1], dev[3])) == -5         # no masked tem_run yet
    plan.tem_run(*dev)
    assert code_of(lambda: plan.tracer_eddy_masked(qd, dev[1], dev[3])) == -5        # no tracer run yet
    with pytest.raises(TypeError):
        plan.tracer_run_masked(qd.float(), dev[1], dev[3])
    plan.tracer_run_masked(qd, dev[1], dev[3])
    plan.tracer_eddy_masked(qd, dev[1], dev[3])
    plan.tem_run(*dev)                                  # new v, omega coefficients: the tracer's are of the run before
    assert code_of(lambda: plan.tracer_eddy_masked(qd, dev[1], dev[3])) == -5
    plan.set_tem(7, 3, plev * 100)
    assert code_of(lambda: plan.tracer_run_masked(qd, dev[1], dev[3])) == -5         # none since temx_plan_set_tem
    assert code_of(lambda: plan.tracer_run(qd, dev[1], dev[3])) == -6                # the refusal of temx.h stands
    # a plan that is not in missing-value mode
    plain = engine.Plan(lat, orc.zm_latitudes(1), 20, device=0)
    plain.set_tem(7, 3, plev * 100)
    clean = [torch.nan_to_num(x, nan=1.0) for x in dev]
    plain.tem_run(*clean)
    assert code_of(lambda: plain.tracer_run_masked(clean[0], clean[1], clean[3])) == -5
    assert code_of(lambda: plain.tracer_eddy_masked(clean[0], clean[1], clean[3])) == -5


def test_repeated_tracer_runs_are_bitwise_identical_and_leave_the_tem_state_alone():
    lat, lon, plev, f, q, _ = case("random", 20, 7, 3, np.float64)
    plan, dev = masked_plan(lat, plev, f, 20)
    res0, zon0 = plan.tem_run(*dev, want_zonal=True)
    cov0 = plan.coverage().clone()
    eddy0 = plan.tem_eddy(*dev)
    qd, tres, tzon, tcov = tracer_out(plan, dev, q)
    _, tres2, tzon2, tcov2 = tracer_out(plan, dev, q)
    assert np.array_equal(tres, tres2, equal_nan=True) and np.array_equal(tzon, tzon2, equal_nan=True)
    assert np.array_equal(tcov, tcov2)
    plan.tracer_eddy_masked(qd, dev[1], dev[3])
    assert torch.equal(plan.coverage(), cov0)
    eddy1 = plan.tem_eddy(*dev)
    for n in eddy0:
        assert np.array_equal(eddy1[n].cpu().numpy(), eddy0[n].cpu().numpy(), equal_nan=True), n
    res1, zon1 = plan.tem_run(*dev, want_zonal=True)
    assert np.array_equal(res1.cpu().numpy(), res0.cpu().numpy(), equal_nan=True)
    assert np.array_equal(zon1.cpu().numpy(), zon0.cpu().numpy(), equal_nan=True)


# ---- front end ------------------------------------------------------------------------------------------------------
def test_frontend_two_masked_tracers_match_the_oracle():
    from pytemdiags_amd import TEMDiagnostics
    lat, lon = grid("cs8")
    nlev, nt, L = 7, 2, 20
    plev, f, q0 = masked_tracer_fields(lat, lon, nlev, nt)
    _, _, q1 = masked_tracer_fields(lat, lon, nlev, nt, gap=False, which=1)
    other = (lat > 40.0)[:, None, None] & (lon < 120.0)[:, None, None] & (plev > 500.0)[None, :, None]
    q1 = np.where(other, np.nan, q1)
    tem = TEMDiagnostics(*f, lat, q=[q0, q1], plev=plev, L=L, debug_level=0, missing="mask", tracer_mask="own")
    assert tem.ntrac == 2 and tem.tracer_mask == "own" and tem.sweep_form == "masked"
    mo = MaskedOracle(*f, lat, plev, L)
    with pytest.raises(RuntimeError, match="qi"):
        tem.tracer_coverage()
    for qi, q in enumerate((q0, q1)):
        to = MaskedTracerOracle(*f, q, lat, plev, L, mo=mo)
        amb = ambiguous(to.coverage) | ambiguous(mo.coverage)
        assert err(np.asarray(tem.tracer_coverage(qi)), to.coverage) <= 1e-9
        for n in TRACER_RESULTS:
            x = np.asarray(getattr(tem, n)(qi))
            assert err(x, to.results[n]) <= 1e-9 and same_nans(x, to.results[n], amb) == 0, (n, qi)
        for n in ("qb", "qpvpb", "dqb_dp"):
            assert err(np.asarray(getattr(tem, n)[qi]), to.zonal[n]) <= 1e-9, (n, qi)
    # the native fields last: the plan holds one tracer at a time, the first is run again behind the getter
    for qi, q in enumerate((q0, q1)):
        to = MaskedTracerOracle(*f, q, lat, plev, L, mo=mo)
        for n in ("qp", "qpvp"):
            x = np.asarray(getattr(tem, n)[qi])
            assert err(x, to.native[n]) <= 1e-9, (n, qi)
            assert np.array_equal(np.isnan(x), np.isnan(to.native[n])), (n, qi)
    assert np.asarray(tem.tracer_coverage(0)).shape == (180, nlev, nt)
    assert float(np.mean(np.asarray(tem.tracer_coverage(0)) < THR)) > float(np.mean(np.asarray(tem.coverage) < THR))


def test_from_model_levels_with_a_masked_tracer_equals_the_constructor_on_interpolated_fields():
    from pytemdiags_amd import TEMDiagnostics, interp_to_pressure
    from test_vertical_host import PLEV37, frontend_case, model_fields
    lat, lon, hyam, hybm, ps, f = frontend_case(nt=2, nlev=72)
    q = model_fields(lat, lon, 72, 2, n=5)[4]
    kw = dict(plev=PLEV37, L=20, debug_level=0, missing="mask", tracer_mask="own")
    outs = interp_to_pressure(list(f) + [q], PLEV37, ps=ps, hyam=hyam, hybm=hybm)
    assert np.isnan(outs[4]).any()                               # targets below ground
    ref = TEMDiagnostics(*outs[:4], lat, q=[outs[4]], **kw)
    a = TEMDiagnostics.from_model_levels(*f, lat, ps=ps, hyam=hyam, hybm=hybm, q=[q], **kw)

    def tm(x):
        return np.ascontiguousarray(np.transpose(x))
    b = TEMDiagnostics.from_model_levels(*[tm(x) for x in f], lat, ps=tm(ps), hyam=hyam, hybm=hybm, q=[tm(q)],
                                         dims=("time", "lev", "ncol"), **kw)
    for tem in (a, b):
        assert tem.ntrac == 1
        for x, y in ((tem._res, ref._res), (tem._tres[0], ref._tres[0]), (tem._tzon[0], ref._tzon[0]),
                     (tem._tcov[0], ref._tcov[0])):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
    assert np.isnan(np.asarray(ref.qb[0])).any() and np.isfinite(np.asarray(ref.etfy())).any()


def test_blocked_masked_tracer_run_matches_the_whole_run():
    from pytemdiags_amd import TEMDiagnostics
    lat, lon = grid("cs8")
    plev, f, q = masked_tracer_fields(lat, lon, 7, 2)
    kw = dict(plev=plev, L=20, debug_level=0, missing="mask", tracer_mask="own")
    ref = TEMDiagnostics(*f, lat, q=q, **kw)
    tem = TEMDiagnostics(*f, lat, q=q, time_block=1, **kw)
    for name, x, y in (("tres", tem._tres[0], ref._tres[0]), ("tcov", tem._tcov[0], ref._tcov[0])):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert x.shape == y.shape and np.array_equal(np.isnan(x), np.isnan(y)), name
        for i in range(x.shape[0] if name == "tres" else 1):
            xi, yi = (x[i], y[i]) if name == "tres" else (x, y)
            assert err(xi, yi) <= 1e-11, (name, i, err(xi, yi))
    assert np.asarray(tem.tracer_coverage()).shape == (180, 7, 2)
    with pytest.raises(RuntimeError, match="time_block"):
        tem.qp
