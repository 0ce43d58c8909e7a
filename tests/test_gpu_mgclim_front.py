"""Masked grouped time means on the MI355X, front end:
``TEMDiagnostics(..., climatology=True, missing="mask", min_group_coverage=v, time_groups=g, time_weights=w)``.

The fixture is cs4 (866 columns) x 6 levels x 7 times at L = 20 under ``test_mgclim_host.front_mask``, labels
[1,0,-1,1,0,1,1], weights [1,.5,3,2,.25,1,0], ``min_coverage = 0.5``, ``min_group_coverage = 0.5``.

Bounds.
  * against the numpy reference (tests/test_mgclim_host.py, masked_grouped_reference): NaN patterns of all three sets and
    of both coverages exactly -- the reference's coverages keep 1e-6 from the threshold, asserted on the reference alone
    in the host file; ``time_coverage`` exactly; values on finite points within ``tol_of(20, dtype)``, the masked mode's
    bound (1e-9 for fp64 fields, 2e-5 for fp32), normalised as ``test_gpu_nclim.compare_finite`` does: transient
    quantities and the four flux-linear results of every set by the TOTAL's maximum.
  * stationary + transient = total for the four flux-linear results where finite: 1e-12.
  * two GPU routes that differ in summation order (one group against the ``min_time_coverage`` object, a group against
    the masked climatology of its own times, blocked against whole, time-major against engine layout): 1e-9, the bound
    test_gpu_nclim holds between such routes; NaN patterns and counts exactly.  NaN-free input against the unmasked
    grouped climatology: 1e-11, the bound of the corresponding NaN-free tests.  One block: bit for bit."""
import numpy as np
import pytest

from test_gclim_host import LABELS, LINEAR, WEIGHTS
from test_gpu_clim import as_dicts, tensors
from test_gpu_missing import tol_of
from test_mgclim_host import front_fixture, masked_grouped_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
SETS = ("total", "stationary", "transient")
THR, GTHR, L = 0.5, 0.5, 20
_cache = {}


def fixture(dtype=np.float64, nan_free=False):
    key = (np.dtype(dtype).name, nan_free)
    if key not in _cache:
        _cache[key] = front_fixture(dtype, nan_free)
    return _cache[key]


def reference(labels=LABELS, weights=WEIGHTS, dtype=np.float64, key="cs4-front"):
    lat, plev, f = fixture(dtype)
    if dtype is not np.float64:
        key = key + "-" + np.dtype(dtype).name
    return masked_grouped_reference(f, lat, plev, L, labels, weights, THR, GTHR, key=key)


def build(dtype=np.float64, fields=None, **kw):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = fixture(dtype)
    kw.setdefault("time_groups", LABELS)
    kw.setdefault("time_weights", WEIGHTS)
    kw.setdefault("min_group_coverage", GTHR)
    return TEMDiagnostics(*(f if fields is None else fields), lat, plev=plev, L=L, debug_level=0, climatology=True,
                          missing="mask", min_coverage=THR, **kw)


def host(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def compare(got, want, total, tol, tag, groups=None):
    """``test_gpu_nclim.compare_finite`` for sets of ``(lat, plev, G)``: the points where both are finite; ``total`` the
    reference's total set, whose maxima normalise the transient set and the four linear results."""
    worst = (0.0, "")
    for s in SETS:
        for n, r in want[s].items():
            x = got[s][n]
            assert x.shape == r.shape and (groups is None or r.shape[-1] == groups), (s, n, x.shape, r.shape)
            fin = np.isfinite(r) & np.isfinite(x)
            base = total[n] if (s == "transient" or n in LINEAR) else r
            den = np.max(np.abs(base[np.isfinite(base)]))
            e = float(np.max(np.abs(x[fin] - r[fin])) / den)
            worst = max(worst, (e, "%s.%s" % (s, n)))
            assert e <= tol, (tag, s, n, e)
    print("%s: worst normalised error %.2e (%s)" % (tag, worst[0], worst[1]))
    return worst[0]


def same_nans(got, want, tag):
    nans = 0
    for s in SETS:
        assert set(got[s]) == set(want[s]) and len(want[s]) == 26
        for n, r in want[s].items():
            assert np.array_equal(np.isnan(got[s][n]), np.isnan(r)), (tag, s, n, int((np.isnan(got[s][n]) != np.isnan(r)).sum()))
            assert not np.isinf(got[s][n]).any(), (tag, s, n)
            nans += int(np.isnan(r).sum())
    return nans


def group_of(d, g):
    return {s: {n: v[..., g:g + 1] for n, v in d[s].items()} for s in SETS}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_masked_grouped_climatology_matches_the_reference(dtype):
    from pytemdiags_amd import climatology
    tem, ref = build(dtype), reference(dtype=dtype)
    cl = tem.climatology
    assert isinstance(cl, climatology.TEMClimatology) and cl.nt == 7 and cl.time_sum_path == "kernel"
    assert tem.min_group_coverage == GTHR and tem.min_time_coverage is None and tem.sweep_form == "masked"
    assert cl.group_names == [0, 1] and cl.group_counts.tolist() == [2, 4] and cl.group_weights.tolist() == [0.75, 4.0]
    tol = tol_of(L, dtype)
    assert np.abs(ref["full"].coverage - THR).min() >= 1e-6 and np.nanmin(np.abs(ref["stat"].coverage - THR)) >= 1e-6
    tc, sc = host(cl.time_coverage), host(cl.stationary_coverage)
    assert tc.shape == sc.shape == (180, 6, 2)
    assert np.array_equal(tc, ref["time_coverage"])                       # counts over n_g: exact
    assert np.array_equal(np.isnan(sc), np.isnan(ref["stat"].coverage))
    fin = np.isfinite(sc)
    assert np.max(np.abs(sc[fin] - ref["stat"].coverage[fin])) <= tol
    got, want = as_dicts(tensors(cl)), ref["values"]
    assert same_nans(got, want, "reference")
    compare(got, want, want["total"], tol, "cs4 %s" % np.dtype(dtype).name, groups=2)
    # stationary + transient = total for the four results that are linear and homogeneous in the fluxes, where finite
    for n in LINEAR:
        S, T, tot = got["stationary"][n], got["transient"][n], got["total"][n]
        fin = np.isfinite(S) & np.isfinite(T) & np.isfinite(tot)
        assert fin.any()
        e = float(np.max(np.abs(S + T - tot)[fin]) / np.max(np.abs(tot[fin])))
        assert e <= 1e-12, (n, e)
    for n in ("ub", "vb", "thetab", "wapb"):                              # the sets share the mean state
        assert np.array_equal(got["total"][n], got["stationary"][n], equal_nan=True)
        assert np.array_equal(got["total"][n], got["transient"][n], equal_nan=True)
    assert cl.total.epfy().shape == (180, 6, 2) and cl.total.epfy().dtype == dtype and cl.time_coverage.dtype == np.float64


def test_time_weights_alone_give_one_weighted_masked_group():
    lat, plev, f = fixture()
    w = np.array([1, .5, 3, 2, .25, 1, 0])
    tem = build(time_groups=None, time_weights=w)
    ref = masked_grouped_reference(f, lat, plev, L, np.zeros(7, dtype=int), w, THR, GTHR, key="cs4-front-weights")
    cl = tem.climatology
    assert cl.group_counts.tolist() == [7] and ref["need"].tolist() == [4]
    got, want = as_dicts(tensors(cl)), ref["values"]
    assert same_nans(got, want, "weights alone")
    assert np.array_equal(host(cl.time_coverage), ref["time_coverage"])
    compare(got, want, want["total"], tol_of(L, np.float64), "time_weights alone", groups=1)


def test_one_group_of_all_times_is_the_masked_climatology():
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = fixture()
    kw = dict(plev=plev, L=L, debug_level=0, climatology=True, missing="mask", min_coverage=THR)
    old = TEMDiagnostics(*f, lat, min_time_coverage=GTHR, **kw)
    new = build(time_groups=np.zeros(7, dtype=int), time_weights=None)
    want, got = as_dicts(tensors(old.climatology)), as_dicts(tensors(new.climatology))
    assert same_nans(got, want, "one group")
    compare(got, want, want["total"], 1e-9, "one group against min_time_coverage", groups=1)
    assert np.array_equal(host(new.climatology.time_coverage), host(old.climatology.time_coverage))
    # (the indicator of the mean fields is the same in both routes, so the coverage of the stationary run is too)
    assert np.array_equal(host(new.climatology.stationary_coverage), host(old.climatology.stationary_coverage), equal_nan=True)


def test_each_group_is_the_masked_climatology_of_its_own_times():
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = fixture()
    both = build(time_weights=None)
    got = as_dicts(tensors(both.climatology))
    tc, sc = host(both.climatology.time_coverage), host(both.climatology.stationary_coverage)
    kw = dict(plev=plev, L=L, debug_level=0, climatology=True, missing="mask", min_coverage=THR, min_time_coverage=GTHR)
    for g in range(2):
        idx = np.nonzero(LABELS == g)[0]
        own = TEMDiagnostics(*[np.ascontiguousarray(x[..., idx]) for x in f], lat, **kw)
        want = as_dicts(tensors(own.climatology))
        mine = group_of(got, g)
        assert same_nans(mine, want, "group %d" % g)
        compare(mine, want, want["total"], 1e-9, "group %d against the climatology of its own times" % g, groups=1)
        assert np.array_equal(tc[..., g:g + 1], host(own.climatology.time_coverage))
        assert np.array_equal(np.isnan(sc[..., g:g + 1]), np.isnan(host(own.climatology.stationary_coverage)))
        fin = np.isfinite(sc[..., g:g + 1])
        assert np.max(np.abs(sc[..., g:g + 1][fin] - host(own.climatology.stationary_coverage)[fin])) <= 1e-9


def test_nan_free_input_with_the_new_keyword_equals_the_grouped_climatology():
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = fixture(nan_free=True)
    plain = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, climatology=True, time_groups=LABELS, time_weights=WEIGHTS)
    tem = build(fields=f)
    want, got = as_dicts(tensors(plain.climatology)), as_dicts(tensors(tem.climatology))
    assert all(np.all(np.isfinite(v)) for s in SETS for v in got[s].values())
    compare(got, want, want["total"], 1e-11, "NaN-free against the grouped climatology", groups=2)
    assert np.all(host(tem.climatology.time_coverage) == 1.0)
    assert np.max(np.abs(host(tem.climatology.stationary_coverage) - 1.0)) <= 1e-11


@pytest.mark.parametrize("source", ["device", "host-time-major"])
def test_blocked_masked_grouped_climatology_against_the_whole_run(source):
    """The mask varies per snapshot and the groups interleave, so sums, weights and counts cross block boundaries."""
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = fixture()
    whole = build()
    want = as_dicts(tensors(whole.climatology))
    if source == "device":
        args, kw = [torch.as_tensor(x, device=DEV) for x in f], {}
    else:
        args, kw = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in f], {"dims": ("time", "plev", "ncol")}
    kw.update(plev=plev, L=L, debug_level=0, climatology=True, missing="mask", min_coverage=THR, min_group_coverage=GTHR,
              time_groups=LABELS, time_weights=WEIGHTS)
    two = TEMDiagnostics(*args, lat, time_block=2, **kw)
    assert two.climatology.nt == 7
    got = as_dicts(tensors(two.climatology))
    assert same_nans(got, want, "time_block=2")
    compare(got, want, want["total"], 1e-9, "time_block=2 from %s" % source, groups=2)
    assert np.array_equal(host(two.climatology.time_coverage), host(whole.climatology.time_coverage))
    # the stationary run's coverage is the operator applied to the validity indicator of the group means, and that
    # pattern is fixed by the counts, which are exact, and by wsum > 0: the blocks change no bit of it
    assert np.array_equal(host(two.climatology.stationary_coverage), host(whole.climatology.stationary_coverage), equal_nan=True)
    seven = TEMDiagnostics(*args, lat, time_block=7, **kw)
    for s, (res, zon) in tensors(seven.climatology).items():
        assert res.tobytes() == tensors(whole.climatology)[s][0].tobytes(), s
        assert zon.tobytes() == tensors(whole.climatology)[s][1].tobytes(), s
    assert host(seven.climatology.stationary_coverage).tobytes() == host(whole.climatology.stationary_coverage).tobytes()
    assert host(seven.climatology.time_coverage).tobytes() == host(whole.climatology.time_coverage).tobytes()


def test_per_snapshot_object_is_that_of_a_masked_run_without_climatology():
    from pytemdiags_amd import TEMDiagnostics, _lib
    lat, plev, f = fixture()
    plain = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, missing="mask", min_coverage=THR)
    tem = build()
    assert tem.climatology.nt == 7
    assert tem._res.cpu().numpy().tobytes() == plain._res.cpu().numpy().tobytes()
    assert tem._zon.cpu().numpy().tobytes() == plain._zon.cpu().numpy().tobytes()
    np.testing.assert_array_equal(tem.coverage, plain.coverage)
    for n in _lib.RESULT_NAMES:
        np.testing.assert_array_equal(getattr(tem, n)(), getattr(plain, n)())
    np.testing.assert_array_equal(tem.up, plain.up)               # the plan's state is that of the ordinary run
    np.testing.assert_array_equal(tem.vptp, plain.vptp)
    for (a0, a1, a), (b0, b1, b) in zip(tem.iter_native(chunk_cols=512), plain.iter_native(chunk_cols=512)):
        assert (a0, a1) == (b0, b1)
        for n in a:
            np.testing.assert_array_equal(a[n], b[n])


def test_from_model_levels_passes_the_keywords_through():
    """The target levels reach below the surface, so the NaN arise from the remap itself."""
    from test_vertical_host import PLEV37, frontend_case, hybrid_pressure
    from pytemdiags_amd import TEMDiagnostics, interp_to_pressure
    lat, lon, hyam, hybm, ps, f = frontend_case(nt=3)
    p = hybrid_pressure(hyam, hybm, ps)
    levels = PLEV37[(PLEV37 * 100.0 >= p[:, 0, :].max()) & (PLEV37 >= 100.0)]
    kw = dict(L=L, debug_level=0, climatology=True, missing="mask", min_coverage=THR, min_group_coverage=GTHR,
              time_groups=[0, 1, 0], time_weights=[1.0, 2.0, 0.5])
    a = TEMDiagnostics.from_model_levels(*f, lat, plev=levels, ps=ps, hyam=hyam, hybm=hybm, **kw)
    g = interp_to_pressure(f, levels, ps=ps, hyam=hyam, hybm=hybm)
    assert np.isnan(g[0]).any() and not np.isnan(g[0]).all()
    b = TEMDiagnostics(*g, lat, plev=levels, **kw)
    assert a.climatology.nt == b.climatology.nt == 3 and a.min_group_coverage == GTHR
    assert a.climatology.group_counts.tolist() == [2, 1]
    ta, tb = tensors(a.climatology), tensors(b.climatology)
    for s in SETS:
        assert ta[s][0].tobytes() == tb[s][0].tobytes() and ta[s][1].tobytes() == tb[s][1].tobytes(), s
    assert host(a.climatology.time_coverage).tobytes() == host(b.climatology.time_coverage).tobytes()
    assert np.isnan(tb["total"][0]).any() and np.isfinite(tb["total"][0]).any()
    # time-major model levels, fed by a block source
    tm = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in f]
    c = TEMDiagnostics.from_model_levels(*tm, lat, plev=levels, ps=np.ascontiguousarray(ps.T), hyam=hyam, hybm=hybm,
                                         dims=("time", "lev", "ncol"), **kw)
    assert c.climatology.nt == 3
    want, got = as_dicts(tb), as_dicts(tensors(c.climatology))
    assert same_nans(got, want, "time-major")
    compare(got, want, want["total"], 1e-9, "time-major model levels", groups=2)
    assert np.array_equal(host(c.climatology.time_coverage), host(b.climatology.time_coverage))
    assert np.array_equal(host(c.climatology.stationary_coverage), host(b.climatology.stationary_coverage), equal_nan=True)
    assert host(a.climatology.stationary_coverage).tobytes() == host(b.climatology.stationary_coverage).tobytes()


def test_month_groups_on_a_datetime_axis_are_the_same_labels_as_integers():
    from pytemdiags_amd import climatology
    time = np.array(["2001-01-10", "2001-01-20", "2001-02-05", "2001-03-01", "2001-02-15", "2001-03-11", "2001-03-21"],
                    dtype="datetime64[D]")
    by_name = build(time_groups="month", time_weights=None, time=time)
    labels, names = climatology.calendar_groups(time, "month")
    g = climatology.resolve_groups(labels, None, 7, time)
    cl = by_name.climatology
    assert cl.group_names == names == ["Jan", "Feb", "Mar"] and cl.group_counts.tolist() == g.counts.tolist() == [2, 2, 3]
    assert np.array_equal(cl.time, g.time) and cl.group_weights.tolist() == g.wsum.tolist()
    by_int = build(time_groups=labels, time_weights=None, time=time)
    ta, tb = tensors(cl), tensors(by_int.climatology)
    for s in SETS:
        assert ta[s][0].tobytes() == tb[s][0].tobytes() and ta[s][1].tobytes() == tb[s][1].tobytes(), s
    assert host(cl.time_coverage).tobytes() == host(by_int.climatology.time_coverage).tobytes()
    assert host(cl.time_coverage).shape == (180, 6, 3)
