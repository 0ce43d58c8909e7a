"""EP flux by time scale on the MI355X through the paths of the front end that tests/test_gpu_timebands.py does not take:
the time-major constructor (re-layout kernel and torch copy) in front of the band run, the one-block branch of
``_run_blocked`` under ``from_model_levels(..., dims=(time, lev, ncol))``, a record of one valid time, four bands with the
widest filter and the deepest padding, a NaN and an inf in a banded run and the plan after them, ``timebands.filter_time``
called directly, weights given as tensors, and a ``datetime64`` time coordinate.

Grid, restatement and bounds are those of tests/test_gpu_timebands.py, imported (``case``, ``build``, ``bands``,
``check_sets``, ``set_values``, ``host``, ``band_fields``, ``np_filter``): ne4 x 3 levels, L = 12; ``TOL64 = 1e-10`` and
``TOL32 = 2e-5`` field-normalised, ``TOL_ADD = 1e-10`` for additivity.  Wherever two GPU paths are claimed equal, the 26
quantities of every set and of the residual are compared with ``np.array_equal`` (``same_sets``), never within a bound.

Measured on the MI355X (every case prints its own):
  3  one valid time          sets 1.2e-13 (residual.dpsicoslat_dlat)
  4  four bands, nw = 255    fp64: fluxes 3.2e-13 (b.vptpb), sets 3.8e-13 (residual.dpsicoslat_dlat), additivity 1.4e-15
                             fp32: fluxes 5.8e-8 (d.upvpb), sets 5.2e-7 (a.epdiv), additivity 7.0e-8
Everything else in this file is bitwise, and held.  In 5 it is ``timebands.Builder.run`` that raises."""
import numpy as np
import pytest

import test_gpu_tfilt as tf
from conftest import fieldnorm_err
from oracle import tem_oracle as orc
from test_gpu_timebands import (ADDITIVE, FLUXES, L, NLEV, NT, TOL32, TOL64, TOL_ADD, ZM7, band_fields, bands, build, case, check_sets,
                                host, np_filter, set_values, tem_of)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
TM = ("time", "plev", "ncol")
_cache = {}


def _tm(x):
    """[ncol][nlev][nt] -> time-major [nt][nlev][ncol] (or [ncol][nt] -> [nt][ncol]), C-contiguous."""
    return np.ascontiguousarray(np.transpose(x))


def _dev(x):
    return torch.tensor(x, device=DEV)                               # (a copy: the cached fields are read-only)


def same_sets(a, b, tag):
    """Two band objects hold the same bits: the 26 quantities of every set and of the residual."""
    assert a.names == b.names and a.half_width == b.half_width and np.array_equal(a.weights, b.weights), tag
    for s in a.names + ("residual",):
        ra = set_values(a.residual if s == "residual" else a[s])
        rb = set_values(b.residual if s == "residual" else b[s])
        assert len(ra) == len(rb) == 26
        for n in ra:
            assert np.array_equal(ra[n], rb[n]), (tag, s, n)


def same_results(a, b, tag):
    va, vb = set_values(a), set_values(b)
    assert len(va) == 26
    for n in va:
        assert np.array_equal(va[n], vb[n]), (tag, n)


def reference(f, lat, plev, table, names, dtype):
    """The restatement of tests/test_gpu_timebands.py (``case``) for any record and any padded table: (fluxes by set,
    sets by set), the residual among them."""
    nt = f[0].shape[-1]
    h = (table.shape[1] - 1) // 2
    f64 = [np.asarray(x, dtype=np.float64) for x in f]
    dts = dict(ua_dtype=f[0].dtype, va_dtype=f[1].dtype, wap_dtype=f[3].dtype)
    full = orc.TEMOracle(*f64, lat, plev, L=L, mode="factorised")
    zm = {n: np.asarray(getattr(full, n), dtype=np.float64)[..., h:nt - h] for n in ZM7}
    flux, sets = {}, {}
    rest = {n: zm[n].copy() for n in FLUXES}
    for b, name in enumerate(names):
        filt = [np_filter(x, table[b], dtype).astype(np.float64) for x in f64]
        o = orc.TEMOracle(*filt, lat, plev, L=L, mode="factorised")
        flux[name] = {n: np.asarray(getattr(o, n), dtype=np.float64) for n in FLUXES}
        for n in FLUXES:
            rest[n] -= flux[name][n]
    flux["residual"] = rest
    for name, fl in flux.items():
        sets[name] = orc.TEMOracle.from_zonal_means({**zm, **fl}, full.plev, **dts)
    return flux, sets


# ---- 1. the time-major constructor ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate,path", [(True, "relayout"), (False, "torch")])
def test_time_major_constructor_in_front_of_the_band_run(gate, path, monkeypatch):
    """``dims=(time, plev, ncol)`` with the re-layout kernel (``layout.WHOLE_RUN_KERNEL`` on, as
    tests/test_gpu_time_major.py switches it) and with the torch copy (off), from host arrays, device tensors and with
    descending ``plev``: ordinary results and band sets hold the bits of the engine-layout object."""
    from pytemdiags_amd import TEMDiagnostics, layout
    monkeypatch.setattr(layout, "WHOLE_RUN_KERNEL", {"float64": gate, "float32": gate})
    lat, lon, plev, f, _, h, _ = case()
    ref = tem_of()
    ftm = [_tm(x) for x in f]
    desc = [np.ascontiguousarray(x[:, ::-1, :]) for x in ftm]
    kw = dict(dims=TM, L=L, debug_level=0, time_bands=bands())
    runs = {"host": TEMDiagnostics(*ftm, lat, plev=plev, **kw),
            "device": TEMDiagnostics(*[_dev(x) for x in ftm], lat, plev=plev, **kw),
            "descending": TEMDiagnostics(*desc, lat, plev=plev[::-1].copy(), **kw),
            "descending device": TEMDiagnostics(*[_dev(x) for x in desc], lat, plev=plev[::-1].copy(), **kw)}
    for tag, tem in runs.items():
        assert tem.input_path == path, (tag, tem.input_path)
        assert (tem.NCOL, tem.NLEV, tem.NT) == (lat.size, NLEV, NT) and tem.plev[0] < tem.plev[-1]
        same_results(tem, ref, tag)
        same_sets(tem.bands, ref.bands, tag)
        assert np.array_equal(tem.bands.time, np.arange(NT)[h:NT - h])
    assert isinstance(runs["device"].bands["low"].epfy(), torch.Tensor) and isinstance(runs["host"].bands["low"].epfy(), np.ndarray)


# ---- 2. the one-block branch of _run_blocked ---------------------------------------------------------------------------------
def _levels_case():
    """The fields of ``case`` taken as model-level fields on hybrid levels whose pressure lies up to 3 % above the target
    levels and moves with the surface pressure, which stays above the lowest target (a target below the surface would
    come out NaN); ``edge="hold"``: the target above a column's top holds the column's end."""
    if "levels" not in _cache:
        lat, lon, plev, f, _, _, _ = case()
        s = np.array([0.2, 0.5, 0.9])
        hyam, hybm = plev * 100.0 / 1e5 * (1 - s), plev * 100.0 / 1e5 * s
        t = np.arange(NT)[None, :]
        ps = np.ascontiguousarray(1.02e5 * (1 + 0.01 * np.sin(np.deg2rad(lat))[:, None] * np.cos(0.3 * t + np.deg2rad(lon)[:, None])))
        pm = np.ascontiguousarray(hyam[None, :, None] * 1e5 + hybm[None, :, None] * ps[:, None, :])
        q = np.ascontiguousarray(1e-3 * (1 + 0.1 * np.asarray(f[0]) / 30.0))
        _cache["levels"] = (hyam, hybm, ps, pm, q)
    return _cache["levels"]


@pytest.mark.parametrize("source", ["hybrid", "p_model", "hybrid+q"])
def test_time_major_model_levels_build_the_bands_in_the_one_block_branch(source):
    """``from_model_levels(..., dims=(time, lev, ncol), time_bands=)`` feeds a block source: the bands are built in
    ``_run_blocked``.  Against the same call in engine order, held to the comparison that
    ``test_time_major_whole_run_equals_the_engine_order_run`` of tests/test_gpu_ingest.py applies to the ordinary
    results: bits (``np.array_equal`` of results, zonal intermediates and the device fields)."""
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, _, h, _ = case()
    hyam, hybm, ps, pm, q = _levels_case()
    kw = dict(plev=plev, interp="linear", edge="hold", L=L, debug_level=0, time_bands=bands())
    eng, tmj = dict(kw), dict(kw)
    if source == "p_model":
        eng.update(p_model=pm)
        tmj.update(p_model=_tm(pm))
    else:
        eng.update(ps=ps, hyam=hyam, hybm=hybm)
        tmj.update(ps=_tm(ps), hyam=hyam, hybm=hybm)
    if source == "hybrid+q":
        eng.update(q=q)
        tmj.update(q=_tm(q))
    ref = TEMDiagnostics.from_model_levels(*f, lat, **eng)
    tem = TEMDiagnostics.from_model_levels(*[_tm(x) for x in f], lat, dims=("time", "lev", "ncol"), **tmj)
    assert ref.input_path == "torch" and tem.input_path in ("ingest", "relayout+interp"), (ref.input_path, tem.input_path)
    if source == "p_model":
        assert tem.input_path == "relayout+interp"
    assert (tem.NCOL, tem.NLEV, tem.NT) == (lat.size, NLEV, NT)
    assert np.array_equal(tem._res.cpu().numpy(), ref._res.cpu().numpy()) and np.array_equal(tem._zon.cpu().numpy(), ref._zon.cpu().numpy())
    for a, b in zip(tem._dev_fields, ref._dev_fields):
        assert a.dtype == b.dtype and torch.equal(a, b)
    same_sets(tem.bands, ref.bands, source)
    assert tem.bands.names == ("synoptic", "low") and np.array_equal(tem.bands.time, np.arange(NT)[h:NT - h])
    # the native-grid attributes of a whole run exist after it
    assert tuple(tem.ua.shape) == (lat.size, NLEV, NT) and np.array_equal(host(tem.ua), host(ref.ua))
    assert np.array_equal(host(tem.up), host(ref.up)) and host(tem.up).shape == (lat.size, NLEV, NT)
    assert host(tem.bands["low"].epfy()).shape == (180, NLEV, NT - 2 * h)
    if source == "hybrid+q":
        assert tem.ntrac == 1 and np.array_equal(host(tem.etfy()), host(ref.etfy())) and np.array_equal(host(tem.qp[0]), host(ref.qp[0]))


# ---- 3. one valid time -----------------------------------------------------------------------------------------------------
def test_a_record_of_one_valid_time():
    """``NT = 2h + 1 = 13``: the plan is set for ``nt = 1`` in the band run.  Measured on the MI355X: sets 1.2e-13."""
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, table, h, _ = case()
    nt = 2 * h + 1
    f13 = [np.ascontiguousarray(x[..., :nt]) for x in f]
    time = 100.0 + 6.0 * np.arange(nt)
    tem = TEMDiagnostics(*f13, lat, plev=plev, time=time, L=L, debug_level=0, time_bands=bands())
    tb = tem.bands
    _, sets = reference(f13, lat, plev, np.stack([table[n] for n in tb.names]), tb.names, np.float64)
    check_sets(tb, sets, 1, TOL64, "one valid time")
    assert tb.time.shape == (1,) and tb.time[0] == time[6]
    tm = tb.time_mean()
    same_sets(tm, tb, "time mean of one time")         # a mean over one element is exact and the epilogue is the same
    assert np.array_equal(np.asarray(tm.time), [time[6]])


# ---- 4. four bands, the widest filter, the deepest padding -----------------------------------------------------------------
def bands4():
    from pytemdiags_amd.timebands import lanczos
    return {"a": lanczos(255, low=0.05), "b": lanczos(121, low=0.2, high=0.05), "c": lanczos(9, high=0.2), "d": [0.25, 0.5, 0.25]}


@pytest.mark.parametrize("dtype,tol", [(np.float64, TOL64), (np.float32, TOL32)], ids=["fp64", "fp32"])
def test_four_bands_nw_255_and_a_three_weight_band_padded_to_it(dtype, tol):
    """``NT = 260``, six valid times.  Additivity: ``TOL_ADD`` for fp64 inputs, as in tests/test_gpu_timebands.py; fp32
    inputs give ``epfy epfz utendepfd`` rounded to fp32, five terms of 2^-24 each, which is held to the project's fp32
    bound ``TOL32``.  Measured on the MI355X: fluxes 3.2e-13 (fp64) and 5.8e-8 (fp32), sets 3.8e-13 and 5.2e-7,
    additivity 1.4e-15 and 7.0e-8."""
    from pytemdiags_amd import TEMDiagnostics, synth, timebands
    nt, ntv = 260, 6
    lat, lon = synth.cubed_sphere_gll(4)
    plev = synth.pressure_levels(NLEV)
    f = band_fields(lat, lon, plev, nt, dtype=dtype)
    names, table, h = timebands.check_bands(bands4())
    assert names == ("a", "b", "c", "d") and h == 127 and table.shape == (4, 255) and nt - 2 * h == ntv
    assert np.count_nonzero(table[3]) == 3 and np.array_equal(table[3, 126:129], [0.25, 0.5, 0.25])
    tem = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, time_bands=bands4())
    tb = tem.bands
    assert tb.names == names and tb.half_width == h and tb.weights.shape == (4, 255) and np.array_equal(tb.weights, table)
    assert tb.workspace_bytes == 4 * 4 * f[0].shape[0] * NLEV * ntv * f[0].itemsize + 4 * 255 * 8
    assert np.array_equal(tb.time, np.arange(nt)[h:nt - h])
    flux, sets = reference(f, lat, plev, table, names, dtype)
    worst = (0.0, "")
    for name in names:
        for n in FLUXES:
            worst = max(worst, (fieldnorm_err(host(getattr(tb[name], n)), flux[name][n]), name + "." + n))
    print("%s four bands: worst flux error %.2e (%s)" % (np.dtype(dtype).name, worst[0], worst[1]))
    assert worst[0] <= tol, worst
    check_sets(tb, sets, ntv, tol, "%s four bands" % np.dtype(dtype).name)
    for n in ADDITIVE:
        total = host(getattr(tem, n)())[..., h:nt - h]
        s = host(getattr(tb.residual, n)())
        for name in names:
            s = s + host(getattr(tb[name], n)())
        e = fieldnorm_err(s, total)
        print("%s four bands additivity %s: %.2e" % (np.dtype(dtype).name, n, e))
        assert e <= (TOL_ADD if dtype == np.float64 else TOL32), (n, e)
    # padding changes no bit: fma(0, x, acc) == acc for finite x
    x = _dev(f[0])
    padded = timebands.filter_time([x], table[3:4])[0][0]
    short = timebands.filter_time([x], np.array([[0.25, 0.5, 0.25]]))[0][0]
    assert tuple(padded.shape) == (lat.size, NLEV, ntv) and tuple(short.shape) == (lat.size, NLEV, nt - 2)
    assert np.array_equal(tf.bits(padded.cpu().numpy()), tf.bits(short[..., 126:126 + ntv].cpu().numpy()))


# ---- 5. non-finite input ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [(2, float("nan")), (0, float("inf"))], ids=["nan-in-ta", "inf-in-ua"])
def test_a_non_finite_value_raises_in_the_band_run_and_leaves_the_plan_usable(field, value):
    """One NaN in ``ta``, one inf in ``ua``, at an interior (column, level, time): the band run comes first, so it is
    ``timebands.Builder.run`` that raises ``climatology._NAN_MESSAGE`` (the ordinary run's message has the same text; the
    frame that raised tells them apart).  A clean construction on the same grid afterwards, on the cached averager and
    its plan, holds the bits of the object built before the failure."""
    import re

    from pytemdiags_amd import TEMDiagnostics, climatology
    lat, lon, plev, f, _, _, _ = case()
    before = tem_of()
    dirty = [x.copy() for x in f]
    dirty[field][433, 1, 20] = value
    with pytest.raises(RuntimeError, match=re.escape(climatology._NAN_MESSAGE)) as exc:
        TEMDiagnostics(*dirty, lat, plev=plev, L=L, debug_level=0, time_bands=bands())
    last = exc.traceback[-1]
    assert last.name == "run" and str(last.path).endswith("timebands.py"), (last.name, str(last.path))
    after = build(time_bands=bands())
    same_results(after, before, "after a refused record")
    same_sets(after.bands, before.bands, "after a refused record")


# ---- 6. timebands.filter_time itself -----------------------------------------------------------------------------------------
def test_filter_time_called_directly():
    from pytemdiags_amd import _lib, timebands
    nw, w = 9, tf.weights(9, 2)
    ncol, nlev, nt = 21, 2, 60
    nto = nt - nw + 1
    x64, x32 = tf.record("f64", ncol, nlev, nt), tf.record("f32", ncol, nlev, nt)
    ids = tf.row_ids(ncol * nlev)

    def want(kind, b, out32):
        return np.stack([tf.oracle(kind, p, w[b], nto, out32) for p in range(tf.POOL)])[ids].reshape(ncol, nlev, nto)

    def same(a, b):
        a, b = a.cpu().numpy(), (b.cpu().numpy() if isinstance(b, torch.Tensor) else b)
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(tf.bits(a), tf.bits(b))

    # the default out_dtype: fp32 when every field is, fp64 otherwise; against the Fraction oracle
    o32 = timebands.filter_time([x32, x32], w)
    assert len(o32) == 2 and len(o32[0]) == 2 and o32[1][0].dtype == torch.float32 and tuple(o32[1][0].shape) == (ncol, nlev, nto)
    mixed = timebands.filter_time([x32, x64], w)
    assert mixed[0][0].dtype == mixed[0][1].dtype == torch.float64
    for b in range(2):
        assert same(o32[b][0], want("f32", b, True)) and same(o32[b][1], want("f32", b, True))
        assert same(mixed[b][0], want("f32", b, False)) and same(mixed[b][1], want("f64", b, False))
    wide = timebands.filter_time([x32], w, out_dtype=torch.float64)
    assert same(wide[1][0], want("f32", 1, False))
    # weights as numpy, as a CPU tensor and as a device tensor
    for wt in (torch.tensor(w), torch.tensor(w, device=DEV), w.tolist()):
        got = timebands.filter_time([x32, x64], wt)
        assert all(same(got[b][i], mixed[b][i]) for b in range(2) for i in range(2))
    # a permuted view against its contiguous copy
    base = x64.permute(1, 0, 2).contiguous()                  # [nlev][ncol][nt]
    view = base.permute(1, 0, 2)
    assert not view.is_contiguous() and torch.equal(view, x64)
    got = timebands.filter_time([view], w)
    assert all(same(got[b][0], mixed[b][1]) for b in range(2))
    # eight fields are served, nine are refused
    eight = timebands.filter_time([x64, x32] * 4, w)
    assert all(same(eight[b][i], mixed[b][1 - i % 2]) for b in range(2) for i in range(8))
    with pytest.raises(_lib.TemxError, match="nf must lie"):
        timebands.filter_time([x64] * 9, w)
    # refusals of the wrapper and of the library
    with pytest.raises(ValueError, match="one shape"):
        timebands.filter_time([x64, x64[:, :, :-1]], w)
    with pytest.raises(ValueError, match="one shape"):
        timebands.filter_time([x64[0]], w)
    with pytest.raises(ValueError, match=r"\[nb\]\[nw\]"):
        timebands.filter_time([x64], w[0])
    with pytest.raises(_lib.TemxError, match="shorter than the filter"):
        timebands.filter_time([x64[:, :, :8]], w)
    with pytest.raises(_lib.TemxError, match="does not narrow"):
        timebands.filter_time([x32, x64], w, out_dtype=torch.float32)
    again = timebands.filter_time([x32, x64], w)               # and the call is served after the refusals
    assert all(same(again[b][i], mixed[b][i]) for b in range(2) for i in range(2))


# ---- 7. weights given as tensors ----------------------------------------------------------------------------------------------
def test_weights_given_as_tensors():
    ref = tem_of()
    w = bands()
    for tag, conv in (("cpu", lambda a: torch.tensor(a)), ("device", lambda a: torch.tensor(a, device=DEV)),
                      ("grad", lambda a: torch.tensor(a, requires_grad=True))):
        tem = build(time_bands={n: conv(a) for n, a in w.items()})
        assert np.array_equal(tem.bands.weights, ref.bands.weights), tag
        same_sets(tem.bands, ref.bands, tag)
    w32 = {n: torch.tensor(a, dtype=torch.float32) for n, a in w.items()}
    a = build(time_bands=w32)
    b = build(time_bands={n: np.asarray(t.numpy(), dtype=np.float64) for n, t in w32.items()})
    assert not np.array_equal(a.bands.weights, ref.bands.weights) and a.bands.weights.dtype == np.float64
    same_sets(a.bands, b.bands, "fp32 weights")


# ---- 8. a real time coordinate -------------------------------------------------------------------------------------------------
def test_a_datetime64_time_coordinate_reaches_the_bands():
    from pytemdiags_amd import climatology
    time = np.datetime64("2001-01-01T00", "h") + 6 * np.arange(NT).astype("timedelta64[h]")
    assert time.dtype == np.dtype("datetime64[h]")
    tem = build(time=time, time_bands=bands())
    h = tem.bands.half_width
    assert tem.bands.time.dtype == time.dtype and np.array_equal(tem.bands.time, time[h:NT - h])
    tm = tem.bands.time_mean()
    assert np.array_equal(tm.time, climatology.mean_time(time[h:NT - h])) and tm.time.shape == (1,)
    assert tm.time[0] == time[h] + (time[NT - h - 1] - time[h]) // 2
    same_sets(tem.bands, tem_of().bands, "datetime64 time")
