"""Model levels to pressure levels on the MI355X: the two lane maps of temxv_interp against the numpy contract
(test_vertical_host.interp_ref), repeatability, strided inputs, streams, and TEMDiagnostics.from_model_levels
against the constructor on pre-interpolated arrays and against the CPU oracle."""
import numpy as np
import pytest

from oracle import tem_oracle as orc
from test_vertical_host import (PLEV37, assert_no_edge_ties, case_ne8, frontend_case, hybrid_levels, hybrid_pressure,
                                inside_everywhere, interp_ref, model_fields)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RESULTS = ("vtem", "omegatem", "wtem", "psitem", "epfy", "epfz", "epdiv", "utendepfd", "utendvtem", "utendwtem")
TRACER_RESULTS = ("etfy", "etfz", "etdiv", "qtendetfd", "qtendvtem", "qtendwtem")
PT = PLEV37 * 100.0


def check(out, ref, dtype, what):
    """Identical NaN pattern everywhere, and over finite values
      fp64 fields  max|d| <= 1e-12 max|ref|.  Derived, not measured: a weight moves by at most a few ulps of the
                   logarithms times ln p / d ln p (below 300 for these levels, 143 on 72 of them), about 6e-14; times
                   a level difference of at most 2 max|x| that is about 1.3e-13; the bound leaves about 8x over it.
      fp32 fields  one final rounding of the fp64 result: <= 2^-23 max|ref| against the reference rounded the same way."""
    out = np.asarray(out)
    assert out.dtype == dtype and out.shape == ref.shape, what
    if dtype == np.float32:
        ref = ref.astype(np.float32)
    assert np.array_equal(np.isnan(out), np.isnan(ref)), (what, int(np.count_nonzero(np.isnan(out) != np.isnan(ref))))
    fin = np.isfinite(ref)
    assert fin.any() and np.all(np.isfinite(out[fin])), what
    d = float(np.max(np.abs(out[fin].astype(np.float64) - ref[fin].astype(np.float64))))
    scale = float(np.max(np.abs(ref[fin])))
    bound = (1e-12 if dtype == np.float64 else 2.0 ** -23) * scale
    print("%s: max|d| = %.3e, bound %.3e" % (what, d, bound))
    assert d <= bound, (what, d, bound)


def problem(nt, nlev=72, nf=4, dtype=np.float64, seed=5):
    """The ne8 fixture; every third column of it for long rows (the reference is a Python loop over columns and times):
    3458 and 1153 columns are a multiple of no tile of either lane map."""
    lat, lon, hyam, hybm, ps = case_ne8(nt=nt, nlev=nlev)
    if nt >= 30:
        lat, lon, ps = lat[::3], lon[::3], ps[::3]
    f = model_fields(lat, lon, nlev, nt, n=nf, seed=seed, dtype=dtype)
    return lat, lon, hyam, hybm, ps, f


# nt = 1 and 3 take the slab-staged map, 30 and 91 lanes along time; both have ragged tails.
@pytest.mark.parametrize("nt", [1, 3, 30, 91])
@pytest.mark.parametrize("dtype,nf,nlev,ps_dtype,method,edge", [
    (np.float64, 4, 72, np.float64, "log", "nan"),
    (np.float32, 4, 72, np.float32, "log", "nan"),
    (np.float64, 1, 72, np.float32, "linear", "hold"),
    (np.float64, 6, 128, np.float64, "log", "hold"),
    (np.float32, 6, 128, np.float64, "linear", "nan"),
])
def test_hybrid_parity(nt, dtype, nf, nlev, ps_dtype, method, edge):
    from pytemdiags_amd import interp_to_pressure
    lat, lon, hyam, hybm, ps, f = problem(nt, nlev, nf, dtype)
    ps = ps.astype(ps_dtype)
    out = interp_to_pressure(f, PLEV37, ps=ps, hyam=hyam, hybm=hybm, method=method, edge=edge)
    assert isinstance(out, list) and len(out) == nf
    ps64 = ps.astype(np.float64)                       # the kernel forms p in fp64 from ps as given
    p = hybrid_pressure(hyam, hybm, ps64)
    assert_no_edge_ties(p, PT)
    for i in range(nf):
        ref = interp_ref(f[i], p, PT, method, edge, psurf=ps64)
        check(out[i], ref, dtype, "hybrid nt=%d f%d %s %s" % (nt, i, method, edge))
    assert np.isnan(out[0]).any()                      # some targets are below ground


@pytest.mark.parametrize("nt", [1, 3, 30, 91])
@pytest.mark.parametrize("dtype,p_dtype,method,edge", [(np.float64, np.float64, "log", "hold"),
                                                       (np.float32, np.float32, "log", "nan"),
                                                       (np.float32, np.float64, "linear", "hold")])
def test_field_pressure_parity(nt, dtype, p_dtype, method, edge):
    from pytemdiags_amd import interp_to_pressure
    lat, lon, hyam, hybm, ps, f = problem(nt, 72, 4, dtype, seed=9)
    p = hybrid_pressure(hyam, hybm, ps).astype(p_dtype)
    p64 = p.astype(np.float64)
    assert_no_edge_ties(p64, PT)                       # the fixture's condition, for the pressures the kernel sees
    out = interp_to_pressure(f, PLEV37, p=p, method=method, edge=edge)
    for i in range(4):
        check(out[i], interp_ref(f[i], p64, PT, method, edge), dtype, "field nt=%d f%d %s %s" % (nt, i, method, edge))


@pytest.mark.parametrize("nt", [2, 40])
def test_bad_columns_nan_values_and_targets_above_the_top(nt):
    from pytemdiags_amd import interp_to_pressure
    lat, lon, hyam, hybm, ps, f = problem(nt, 72, 2)
    p = hybrid_pressure(hyam, hybm, ps)
    p[11, 40, 1] = p[11, 39, 1]                        # not strictly increasing
    p[12, 5, 0] = np.nan
    p[13, 71, 1] = np.inf
    f[0][20, 50, 1] = np.nan                           # reaches two brackets of one column
    plev = np.concatenate([[0.05], PLEV37])            # 0.05 hPa: above the model top
    for edge in ("nan", "hold"):
        out = interp_to_pressure(f, plev, p=p, edge=edge)
        for i in range(2):
            ref = interp_ref(f[i], p, plev * 100.0, "log", edge)
            check(out[i], ref, np.float64, "bad columns nt=%d f%d %s" % (nt, i, edge))
        assert np.all(np.isnan(out[1][11, :, 1])) and np.all(np.isnan(out[1][12, :, 0])) and np.all(np.isnan(out[1][13, :, 1]))
        assert np.isfinite(out[1][0, 0, 0]) == (edge == "hold")
    # hybrid: a column without a surface pressure is NaN, its neighbours are not touched
    ps2 = ps.copy()
    ps2[30, 0] = np.nan
    out = interp_to_pressure(f[1], PLEV37, ps=ps2, hyam=hyam, hybm=hybm)
    ref = interp_ref(f[1], hybrid_pressure(hyam, hybm, ps2), PT, psurf=ps2)
    check(out, ref, np.float64, "NaN surface pressure nt=%d" % nt)
    assert np.all(np.isnan(out[30, :, 0])) and np.isfinite(out[29, 10, 0]) and np.isfinite(out[31, 10, 0])


def test_lane_maps_agree_bit_for_bit(monkeypatch):
    """Both maps run the same walk on the same numbers: where both apply, the results are the same bits."""
    from pytemdiags_amd import interp_to_pressure
    for nt, dtype, nf in ((3, np.float64, 4), (8, np.float32, 4), (16, np.float64, 2)):
        lat, lon, hyam, hybm, ps, f = problem(nt, 72, nf, dtype)
        got = {}
        for m in ("time", "slab"):
            monkeypatch.setenv("TEMXV_MAP", m)
            got[m] = interp_to_pressure(f, PLEV37, ps=ps, hyam=hyam, hybm=hybm, edge="hold")
        monkeypatch.delenv("TEMXV_MAP")
        for a, b in zip(got["time"], got["slab"]):
            assert np.array_equal(a, b, equal_nan=True), (nt, dtype)


def test_repeats_streams_kinds_and_strided_tensors():
    from pytemdiags_amd import LabeledArray, interp_to_pressure
    for nt in (3, 30):
        lat, lon, hyam, hybm, ps, f = problem(nt, 72, 4)
        kw = dict(ps=ps, hyam=hyam, hybm=hybm)
        first = interp_to_pressure(f, PLEV37, **kw)
        again = interp_to_pressure(f, PLEV37[::-1], **kw)              # descending targets come back ascending
        for a, b in zip(first, again):
            assert np.array_equal(a, b, equal_nan=True)
        # device tensors in, device tensors out; a side stream gives the same bits
        dev = [torch.as_tensor(x, device="cuda:0") for x in f]
        psd = torch.as_tensor(ps, device="cuda:0")
        s = torch.cuda.Stream(device="cuda:0")
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            side = interp_to_pressure(dev, PLEV37, ps=psd, hyam=hyam, hybm=hybm)
        s.synchronize()
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in side)
        for a, b in zip(first, side):
            assert np.array_equal(a, b.cpu().numpy(), equal_nan=True)
        # non-contiguous views are handled (never read with the wrong strides): a transposed layout, a column slice
        tr = dev[0].permute(2, 0, 1).contiguous().permute(1, 2, 0)
        assert not tr.is_contiguous()
        one = interp_to_pressure(tr, PLEV37, ps=psd, hyam=hyam, hybm=hybm)
        assert np.array_equal(one.cpu().numpy(), first[0], equal_nan=True)
        sl = interp_to_pressure(dev[1][5:-3:2], PLEV37, ps=psd[5:-3:2], hyam=hyam, hybm=hybm)
        assert np.array_equal(sl.cpu().numpy(), first[1][5:-3:2], equal_nan=True)
        # one array in, one array out; 2-d fields; labelled arrays keep their labels
        assert np.array_equal(interp_to_pressure(f[2], PLEV37, **kw), first[2], equal_nan=True)
        two = interp_to_pressure(f[3][:, :, 0], PLEV37, ps=ps[:, 0], hyam=hyam, hybm=hybm)
        assert two.shape == (lat.size, 37) and np.array_equal(two, first[3][:, :, 0], equal_nan=True)
        la = LabeledArray(f[0], ("ncol", "lev", "time"), {"time": np.arange(nt) * 6.0}, name="U")
        lo = interp_to_pressure(la, PLEV37[::-1], **kw)
        assert lo.dims == ("ncol", "plev", "time") and lo.name == "U" and np.array_equal(lo.coords["plev"], PLEV37)
        assert np.array_equal(lo.coords["time"], np.arange(nt) * 6.0) and np.array_equal(lo.values, first[0], equal_nan=True)


def test_c_abi_refuses_aliasing_on_the_device():
    """The raw entry point takes dense arrays only and refuses a dst that overlaps a src."""
    import ctypes as C
    from pytemdiags_amd import _vert
    lib = _vert.load()
    hyam, hybm = hybrid_levels(8)
    x = torch.zeros(10 * 8 * 2, dtype=torch.float64, device="cuda:0")
    ps = torch.full((10, 2), 1e5, dtype=torch.float64, device="cuda:0")
    plev = np.array([3e4, 5e4])
    dp = C.POINTER(C.c_double)
    src = (C.c_void_p * 1)(x.data_ptr())
    dst = (C.c_void_p * 1)(x.data_ptr() + 8 * 4)
    rc = lib.temxv_interp(0, 1, src, dst, 0, 10, 8, 2, 2, plev.ctypes.data_as(dp), 0, hyam.ctypes.data_as(dp),
                          hybm.ctypes.data_as(dp), 1e5, C.c_void_p(ps.data_ptr()), 0, 0, 0, None)
    assert rc == -1 and b"overlaps" in lib.temx_last_error()


# ---- front end ----------------------------------------------------------------------------------------------------
def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("missing", ["mask", "raise"])
def test_from_model_levels_equals_constructor_on_interpolated_arrays(missing):
    from pytemdiags_amd import TEMDiagnostics, interp_to_pressure
    lat, lon, hyam, hybm, ps, f = frontend_case()
    levels = PLEV37 if missing == "mask" else PLEV37[inside_everywhere(hybrid_pressure(hyam, hybm, ps), PT)]
    kw = dict(L=30, debug_level=0, missing=missing)
    a = TEMDiagnostics.from_model_levels(*f, lat, plev=levels, ps=ps, hyam=hyam, hybm=hybm, **kw)
    g = interp_to_pressure(f, levels, ps=ps, hyam=hyam, hybm=hybm)
    assert np.isnan(g[0]).any() == (missing == "mask")
    b = TEMDiagnostics(*g, lat, plev=levels, **kw)
    for n in RESULTS:
        x, y = getattr(a, n)(), getattr(b, n)()
        assert isinstance(x, np.ndarray) and x.dtype == y.dtype and same(x, y), n
    assert np.isfinite(a.vtem()).any()
    if missing == "mask":
        assert same(a.coverage, b.coverage) and np.isnan(a.epdiv()).any()
    else:
        assert a.coverage is None and b.coverage is None
    assert same(a.up, b.up) and same(a.ub, b.ub)
    assert np.array_equal(a.plev, levels) and a.NLEV == levels.size


def test_from_model_levels_matches_the_oracle_end_to_end():
    """The 23 levels inside every column: no NaN arises, and the ten results match the CPU oracle run on the numpy
    contract's fields to the fp64 parity tolerance of the pipeline, 1e-10 field-normalised.  The fields are one
    atmosphere sampled at each model level's own pressure (test_vertical_host.frontend_case), which keeps the TEM
    formulas as well conditioned as on the pressure-level fields that tolerance was set on."""
    from conftest import fieldnorm_err
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, hyam, hybm, ps, f = frontend_case()
    p = hybrid_pressure(hyam, hybm, ps)
    levels = PLEV37[inside_everywhere(p, PT)]
    assert levels.size == 23
    tem = TEMDiagnostics.from_model_levels(*f, lat, plev=levels, ps=ps, hyam=hyam, hybm=hybm, L=30, debug_level=0)
    g = [interp_ref(x, p, levels * 100.0, psurf=ps) for x in f]
    assert all(np.all(np.isfinite(x)) for x in g)
    ref = orc.TEMOracle(*g, lat, levels, L=30, mode="factorised")
    for n in RESULTS:
        e = fieldnorm_err(getattr(tem, n)(), getattr(ref, n)())
        print("%s: %.3e" % (n, e))
        assert e <= 1e-10, (n, e)


def test_target_below_ground_raises_like_the_reference():
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, hyam, hybm, ps, f = frontend_case()
    with pytest.raises(RuntimeError, match="Variable has nans"):
        TEMDiagnostics.from_model_levels(*f, lat, plev=PLEV37, ps=ps, hyam=hyam, hybm=hybm, L=30, debug_level=0)
    # held edges do not reach below the surface either
    with pytest.raises(RuntimeError, match="Variable has nans"):
        TEMDiagnostics.from_model_levels(*f, lat, plev=PLEV37, ps=ps, hyam=hyam, hybm=hybm, L=30, debug_level=0,
                                         edge="hold")


def test_from_model_levels_with_tracers():
    from pytemdiags_amd import TEMDiagnostics, interp_to_pressure, synth
    lat, lon, hyam, hybm, ps, f = frontend_case()
    nominal = np.exp(np.linspace(np.log(0.1), np.log(997.6), 72))
    q = [synth.analytic_tracer(lat, lon, nominal, 2, which=i, seed=100 + i) for i in range(2)]
    p = hybrid_pressure(hyam, hybm, ps)
    levels = PLEV37[inside_everywhere(p, PT)]
    a = TEMDiagnostics.from_model_levels(*f, lat, plev=levels, p_model=p, q=q, L=30, debug_level=0, interp="linear")
    g = interp_to_pressure(f + q, levels, p=p, method="linear")
    b = TEMDiagnostics(*g[:4], lat, q=g[4:], plev=levels, L=30, debug_level=0)
    for qi in range(2):
        for n in TRACER_RESULTS:
            assert same(getattr(a, n)(qi), getattr(b, n)(qi)), (n, qi)
    assert same(a.qb[1], b.qb[1]) and same(a.vtem(), b.vtem())
    with pytest.raises(NotImplementedError, match="tracers"):
        TEMDiagnostics.from_model_levels(*f, lat, plev=levels, p_model=p, q=q, L=30, debug_level=0, missing="mask")
