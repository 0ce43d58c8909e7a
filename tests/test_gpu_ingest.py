"""Time-major model-level records on the MI355X: the fused remap ``temxi_records_to_pressure`` against the chain of
re-layout and interpolation (bit for bit) and against the numpy contract (test_vertical_host.interp_ref), its tails,
seams, bad columns and canaries, and ``TEMDiagnostics.from_model_levels(..., dims=(time, lev, ncol))`` as a whole run
and blocked, from device tensors, host arrays, a memmap and CPU tensors.

Bounds.  Fused against chain: the same walk on the same numbers, ``np.array_equal(..., equal_nan=True)``.  Against
``interp_ref``: ``check`` of test_gpu_vertical.py (1e-12 max|ref| fp64, 2^-23 max|ref| fp32, identical NaN pattern),
derived there.  Blocked against whole: the bound tests/test_gpu_time_major.py uses, 1e-11 fp64 and 1e-5 fp32,
field-normalised.  Shapes: 1153 and 3458 columns are a multiple of no tile (16 .. 256 columns)."""
import ctypes as C
import gc

import numpy as np
import pytest

from conftest import fieldnorm_err
from test_gpu_vertical import check
from test_vertical_host import (PLEV37, assert_no_edge_ties, case_ne8, frontend_case, hybrid_pressure,
                                inside_everywhere, interp_ref, model_fields, tie_case)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
PT = PLEV37 * 100.0
_cache = {}


def _tm(x):
    """[ncol][nlev][nt] -> time-major [nt][nlev][ncol] (or [ncol][nt] -> [nt][ncol]), C-contiguous."""
    return np.ascontiguousarray(np.transpose(x))


def _dev(x):
    return torch.as_tensor(x, device=DEV)


def _records(ncol, nlev, nt_src, nf, dtypes, ps_dtype, seed=0):
    """Time-major records with the surface of the ne8 fixture: any numbers will do for a comparison of bits."""
    lat, lon, hyam, hybm, ps = case_ne8(nt=nt_src, nlev=nlev)
    sl = slice(None, None, 3) if ncol == 1153 else slice(None)
    ps = ps[sl]
    assert ps.shape[0] == ncol
    rng = np.random.default_rng(seed)
    srcs = [rng.standard_normal((nt_src, nlev, ncol)).astype(dtypes[i % len(dtypes)]) for i in range(nf)]
    return hyam, hybm, _tm(ps).astype(ps_dtype), srcs


def _both(srcs, ps, plev_pa, hyam, hybm, **kw):
    from pytemdiags_amd import vertical
    d = [_dev(s) for s in srcs]
    psd = _dev(ps)
    fused = vertical.records_to_pressure_device(d, psd, plev_pa, hyam=hyam, hybm=hybm, path="fused", **kw)
    chain = vertical.records_to_pressure_device(d, psd, plev_pa, hyam=hyam, hybm=hybm, path="chain", **kw)
    return [x.cpu().numpy() for x in fused], [x.cpu().numpy() for x in chain]


F64, F32 = np.float64, np.float32
# (source dtypes, ps dtype, method, edge, nf, nlev, target levels [hPa], ntb, ncol)
CASES = [
    ((F64,), F64, "log", "nan", 4, 72, PLEV37, 30, 1153),
    ((F32,), F32, "log", "nan", 4, 72, PLEV37, 17, 3458),
    ((F32, F64), F32, "linear", "hold", 6, 128, PLEV37, 16, 1153),
    ((F64,), F64, "log", "hold", 8, 72, PLEV37, 15, 1153),
    ((F32,), F64, "linear", "nan", 8, 128, PLEV37, 3, 3458),
    ((F32,), F32, "log", "hold", 4, 72, PLEV37, 30, 1153),
    ((F64, F32), F64, "log", "nan", 8, 72, PLEV37, 17, 1153),
    ((F64,), F64, "linear", "hold", 1, 26, np.array([500.0]), 1, 3458),
    ((F32,), F32, "log", "nan", 6, 26, np.array([10.0, 100.0, 500.0, 850.0, 1000.0]), 1, 1153),
    ((F64,), F32, "log", "hold", 1, 26, np.array([10.0, 100.0, 500.0, 850.0, 1000.0]), 3, 1153),
    ((F32,), F64, "log", "nan", 1, 26, np.array([500.0]), 16, 1153),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-ps%s-%s-%s-nf%d-%dto%d-ntb%d-ncol%d" % (
    "+".join(np.dtype(d).name for d in c[0]), np.dtype(c[1]).itemsize * 8, c[2], c[3], c[4], c[5], len(c[6]), c[7], c[8]))
def test_fused_equals_chain_bit_for_bit(case):
    dtypes, ps_dtype, method, edge, nf, nlev, plev, ntb, ncol = case
    t0 = 2
    nt_src = t0 + ntb + 1                                   # both ends of the window are interior
    hyam, hybm, ps, srcs = _records(ncol, nlev, nt_src, nf, dtypes, ps_dtype, seed=nf + ntb)
    fused, chain = _both(srcs, ps, plev * 100.0, hyam, hybm, t0=t0, ntb=ntb, method=method, edge=edge)
    want = np.float32 if set(dtypes) == {F32} else np.float64
    for i in range(nf):
        assert fused[i].dtype == want and fused[i].shape == (ncol, len(plev), ntb)
        assert np.array_equal(fused[i], chain[i], equal_nan=True), (i, int(np.count_nonzero(~(
            (fused[i] == chain[i]) | (np.isnan(fused[i]) & np.isnan(chain[i]))))))
    assert np.isfinite(fused[0]).any()
    if len(plev) > 1:
        assert np.isnan(fused[0]).any()                     # below ground over the plateau and the polar cap


@pytest.mark.parametrize("dtype,ps_dtype,method,edge,ntb", [(F64, F64, "log", "nan", 8), (F32, F32, "log", "hold", 5),
                                                            (F64, F32, "linear", "hold", 3)])
def test_fused_against_the_numpy_contract(dtype, ps_dtype, method, edge, ntb):
    from pytemdiags_amd import vertical
    t0, nt_src = 1, ntb + 2
    lat, lon, hyam, hybm, ps = case_ne8(nt=nt_src, nlev=72)
    lat, lon, ps = lat[::3], lon[::3], ps[::3].astype(ps_dtype)
    assert lat.size == 1153
    f = model_fields(lat, lon, 72, nt_src, n=4, dtype=dtype)
    out = vertical.records_to_pressure_device([_dev(_tm(x)) for x in f], _dev(_tm(ps)), PT, hyam=hyam, hybm=hybm, t0=t0,
                                              ntb=ntb, method=method, edge=edge, path="fused")
    ps64 = ps.astype(np.float64)[:, t0:t0 + ntb]
    p = hybrid_pressure(hyam, hybm, ps64)
    assert_no_edge_ties(p, PT)
    for i in range(4):
        ref = interp_ref(f[i][:, :, t0:t0 + ntb], p, PT, method, edge, psurf=ps64)
        check(out[i].cpu().numpy(), ref, dtype, "ingest f%d %s %s" % (i, method, edge))
    assert np.isnan(out[0].cpu().numpy()).any()


@pytest.mark.parametrize("nlev,nt,nf,ps_dtype", [(26, 2, 4, F64), (13, 1, 4, F64), (26, 2, 8, F32), (26, 5, 1, F64)])
def test_targets_on_every_level_seam_and_on_the_surface(nlev, nt, nf, ps_dtype):
    """The walk is cut at the ring's window seams (every kw-th level; kw depends on nf, dtype and ntb).  Dyadic hyam,
    hybm and ps (tie_case): the targets lie exactly on EVERY level -- so on every seam of whatever tile is chosen --,
    on level 0, on the bottom level and on the surface of the tied columns.  The chain cuts elsewhere (segments of
    vert_slab_shape) or not at all: the bits must agree, every tied target must find its bracket, and the one on level 0
    (weight 0 in the first bracket) must carry that level's own value."""
    ncol = 3 * 131 + 7
    c, _ = tie_case(nlev, nt, ncol, nf=nf, ps_dtype=ps_dtype)
    H = c["H"]
    hs = sorted({4, 995 * 64, *[int(h) for h in H]})
    pt = np.array(hs, dtype=np.float64) / 64.0 * 100.0
    srcs = [_tm(x) for x in c["f"]]
    for method in ("log", "linear"):
        for edge in ("nan", "hold"):
            fused, chain = _both(srcs, _tm(c["ps"]), pt, c["hyam"], c["hybm"], p0=c["p0"], method=method, edge=edge)
            for i in range(nf):
                assert np.array_equal(fused[i], chain[i], equal_nan=True), (method, edge, i)
            # the target on level 0 opens the first bracket with weight 0 (linear: x is p itself): level 0's own value
            star = c["star"]
            if method == "linear":
                assert np.array_equal(fused[0][:, hs.index(int(H[0])), :], c["f"][0][:, 0, :]), edge
            assert np.all(np.isfinite(fused[0][star][:, 1:-1, :]))      # every tied target found its bracket
            j = hs.index(995 * 64)                          # the surface of the tied columns: held, or below the bottom level
            assert np.all(np.isnan(fused[0][star, j, :])) == (edge == "nan")


def test_bad_columns_stay_where_they_are():
    from pytemdiags_amd import _ingest, vertical
    ntb, nlev, ncol = 5, 72, 1153
    hyam, hybm, ps, srcs = _records(ncol, nlev, ntb + 2, 2, (F64,), F64, seed=3)
    ps[3, 500] = np.nan                                     # (time 3, column 500): window time 2
    srcs[1][2, 40, 77] = np.nan                             # window time 1, level 40, column 77
    fused, chain = _both(srcs, ps, PT, hyam, hybm, t0=1, ntb=ntb)
    for a, b in zip(fused, chain):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.all(np.isnan(fused[0][500, :, 2])) and np.all(np.isnan(fused[1][500, :, 2]))
    for i, t in ((499, 2), (501, 2), (500, 1), (500, 3)):
        assert np.isfinite(fused[0][i, 20, t])
    p = hybrid_pressure(hyam, hybm, _tm(ps)[77:78, 1:1 + ntb])[0, :, 1]
    hit = (PT > p[39]) & (PT <= p[41])                      # the two brackets of level 40
    assert hit.any() and np.all(np.isnan(fused[1][77, hit, 1]))
    assert np.array_equal(np.isnan(fused[1][77, :, 1]), np.isnan(fused[0][77, :, 1]) | hit)
    assert np.array_equal(np.isnan(fused[1][77, :, 0]), np.isnan(fused[0][77, :, 0]))
    # hyam decreasing, straight through the C ABI (the front end refuses it): every column NaN, nothing else happens
    lib = _ingest.load()
    d, psd = [_dev(s) for s in srcs[:1]], _dev(ps)
    out = torch.zeros((ncol, 37, ntb), dtype=torch.float64, device=DEV)
    dp = C.POINTER(C.c_double)
    rev_a, rev_b = np.ascontiguousarray(hyam[::-1]), np.ascontiguousarray(hybm[::-1])
    rc = lib.temxi_records_to_pressure(0, 1, (C.c_void_p * 1)(d[0].data_ptr()), (C.c_int * 1)(0),
                                       (C.c_void_p * 1)(out.data_ptr()), 0, ncol, nlev, ntb + 2, 1, ntb, 37,
                                       PT.ctypes.data_as(dp), rev_a.ctypes.data_as(dp), rev_b.ctypes.data_as(dp), 1e5,
                                       C.c_void_p(psd.data_ptr()), 0, 0, 0, None)
    assert rc == 0, lib.temx_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert vertical.FUSED_RECORDS.keys() == {"float64", "float32"}


@pytest.mark.parametrize("dtype,nf,ntb", [(F64, 3, 17), (F32, 5, 33), (F64, 8, 1)])
def test_nothing_is_written_outside_the_destinations(dtype, nf, ntb):
    """The destinations are views in the middle of one canary-filled allocation, back to back with odd gaps."""
    from pytemdiags_amd import vertical
    ncol, nlev, nplev = 1153, 26, 5
    plev = np.array([10.0, 100.0, 500.0, 850.0, 1000.0]) * 100.0
    hyam, hybm, ps, srcs = _records(ncol, nlev, ntb + 3, nf, (dtype,), F64, seed=11)
    n = ncol * nplev * ntb
    gap = 37
    tdt = torch.float64 if dtype == F64 else torch.float32
    canary = -12345.0
    big = torch.full(((n + gap) * nf + gap,), canary, dtype=tdt, device=DEV)
    out = [big[gap + i * (n + gap): gap + i * (n + gap) + n].view(ncol, nplev, ntb) for i in range(nf)]
    d, psd = [_dev(s) for s in srcs], _dev(ps)
    vertical.records_to_pressure_device(d, psd, plev, hyam=hyam, hybm=hybm, t0=2, ntb=ntb, edge="hold", out=out,
                                        path="fused")
    ref = vertical.records_to_pressure_device(d, psd, plev, hyam=hyam, hybm=hybm, t0=2, ntb=ntb, edge="hold", path="chain")
    torch.cuda.synchronize()
    flat = big.cpu().numpy()
    inside = np.zeros(flat.size, dtype=bool)
    for i in range(nf):
        a = gap + i * (n + gap)
        inside[a:a + n] = True
        assert np.array_equal(flat[a:a + n].reshape(ncol, nplev, ntb), ref[i].cpu().numpy(), equal_nan=True)
        assert not np.any(flat[a:a + n] == canary)          # and every element of the window was written
    assert np.all(flat[~inside] == canary)


def test_two_calls_and_another_stream_give_the_same_bits():
    from pytemdiags_amd import vertical
    hyam, hybm, ps, srcs = _records(1153, 72, 20, 6, (F32, F64), F32, seed=21)
    d, psd = [_dev(s) for s in srcs], _dev(ps)
    kw = dict(hyam=hyam, hybm=hybm, t0=1, ntb=17, method="log", edge="hold", path="fused")
    a = vertical.records_to_pressure_device(d, psd, PT, **kw)
    b = vertical.records_to_pressure_device(d, psd, PT, **kw)
    st = torch.cuda.Stream(DEV)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        c = vertical.records_to_pressure_device(d, psd, PT, **kw)
    st.synchronize()
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        x, y, z = x.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy()
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)


# ---- front end ----------------------------------------------------------------------------------------------------
TM = ("time", "lev", "ncol")
NT_BLOCKED, NLEV_BLOCKED = 24, 26


def _same_bits(a, b):
    return torch.equal(a._res, b._res) and torch.equal(a._zon, b._zon)


def _same_nan_bits(x, y):
    return np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)


def _frontend(nt=2, nlev=72, dtype=np.float64):
    key = ("frontend", nt, nlev, np.dtype(dtype).name)
    if key not in _cache:
        lat, lon, hyam, hybm, ps, f = frontend_case(nt=nt, nlev=nlev, dtype=dtype)
        inside = PLEV37[inside_everywhere(hybrid_pressure(hyam, hybm, ps), PT)]
        _cache[key] = (lat, lon, hyam, hybm, ps, f, [_tm(x) for x in f], _tm(ps), inside)
    return _cache[key]


@pytest.mark.parametrize("missing", ["raise", "mask"])
def test_time_major_whole_run_equals_the_engine_order_run(missing):
    """All ten results and sixteen zonal attributes, from host arrays, device tensors and labelled arrays."""
    from pytemdiags_amd import LabeledArray, TEMDiagnostics, vertical
    lat, lon, hyam, hybm, ps, f, ftm, pstm, inside = _frontend()
    levels = PLEV37 if missing == "mask" else inside
    kw = dict(plev=levels, hyam=hyam, hybm=hybm, L=30, debug_level=0, missing=missing)
    ref = TEMDiagnostics.from_model_levels(*f, lat, ps=ps, **kw)
    want = "ingest" if vertical.FUSED_RECORDS["float64"] else "relayout+interp"
    host = TEMDiagnostics.from_model_levels(*ftm, lat, ps=pstm, dims=TM, **kw)
    dev = TEMDiagnostics.from_model_levels(*[_dev(x) for x in ftm], lat, ps=_dev(pstm), dims=("time", "plev", "ncol"), **kw)
    lab = TEMDiagnostics.from_model_levels(*[LabeledArray(x, TM, {"time": np.arange(2) * 6.0}, name=n)
                                             for x, n in zip(ftm, ("U", "V", "T", "OMEGA"))], lat, ps=pstm, **kw)
    for tem in (host, dev, lab):
        assert tem.input_path == want
        assert (tem.NCOL, tem.NLEV, tem.NT) == (lat.size, levels.size, 2) and np.array_equal(tem.plev, levels)
        assert _same_nan_bits(tem._res, ref._res) and _same_nan_bits(tem._zon, ref._zon)
        if missing == "mask":
            assert _same_nan_bits(tem._cov, ref._cov)
        for a, b in zip(tem._dev_fields, ref._dev_fields):
            assert a.dtype == b.dtype and _same_nan_bits(a, b)
    assert isinstance(host.vtem(), np.ndarray) and isinstance(dev.vtem(), torch.Tensor)
    assert lab.vtem().dims == ("lat", "plev", "time") and np.array_equal(lab.time, np.arange(2) * 6.0)
    np.testing.assert_array_equal(host.up, ref.up)              # native attributes exist in a whole run
    np.testing.assert_array_equal(lab.psi.values, ref.psi)
    # engine order named by dims= is the run it always was
    eng = TEMDiagnostics.from_model_levels(*f, lat, ps=ps, dims=("ncol", "lev", "time"), **kw)
    assert _same_nan_bits(eng._res, ref._res) and eng.input_path == ref.input_path == "torch"


@pytest.mark.parametrize("gate", [True, False])
def test_whole_run_follows_the_gate_with_the_same_bits(gate, monkeypatch):
    from pytemdiags_amd import TEMDiagnostics, vertical
    monkeypatch.setattr(vertical, "FUSED_RECORDS", {"float64": gate, "float32": gate})
    for dtype in (np.float64, np.float32):
        lat, lon, hyam, hybm, ps, f, ftm, pstm, inside = _frontend(dtype=dtype)
        kw = dict(plev=inside, hyam=hyam, hybm=hybm, L=30, debug_level=0)
        key = ("ref", np.dtype(dtype).name)
        if key not in _cache:
            _cache[key] = TEMDiagnostics.from_model_levels(*f, lat, ps=ps, **kw)
        tem = TEMDiagnostics.from_model_levels(*ftm, lat, ps=pstm, dims=TM, **kw)
        assert tem.input_path == ("ingest" if gate else "relayout+interp")
        assert _same_bits(tem, _cache[key]) and tem.vtem().dtype == dtype


def test_time_major_tracers_and_p_model():
    from pytemdiags_amd import TEMDiagnostics, _lib, synth
    lat, lon, hyam, hybm, ps, f, ftm, pstm, inside = _frontend()
    nominal = np.exp(np.linspace(np.log(0.1), np.log(997.6), 72))
    q = [synth.analytic_tracer(lat, lon, nominal, 2, which=i, seed=100 + i) for i in range(2)]
    kw = dict(plev=inside, L=30, debug_level=0)
    a = TEMDiagnostics.from_model_levels(*f, lat, ps=ps, hyam=hyam, hybm=hybm, q=q, **kw)
    b = TEMDiagnostics.from_model_levels(*ftm, lat, ps=pstm, hyam=hyam, hybm=hybm, q=[_tm(x) for x in q], dims=TM, **kw)
    assert b.ntrac == 2 and _same_bits(a, b)
    for qi in range(2):
        for n in _lib.TRACER_RESULT_NAMES:
            np.testing.assert_array_equal(getattr(a, n)(qi), getattr(b, n)(qi))
        np.testing.assert_array_equal(a.qb[qi], b.qb[qi])
    with pytest.raises(NotImplementedError, match="tracers"):
        TEMDiagnostics.from_model_levels(*ftm, lat, ps=pstm, hyam=hyam, hybm=hybm, q=[_tm(x) for x in q], dims=TM,
                                         missing="mask", **kw)
    # the pressure of every point, time-major like the fields: the chain, in field mode
    p = hybrid_pressure(hyam, hybm, ps)
    c = TEMDiagnostics.from_model_levels(*f, lat, p_model=p, interp="linear", **kw)
    d = TEMDiagnostics.from_model_levels(*ftm, lat, p_model=_tm(p), interp="linear", dims=TM, **kw)
    e = TEMDiagnostics.from_model_levels(*[_dev(x) for x in ftm], lat, p_model=_dev(_tm(p)), interp="linear", dims=TM, **kw)
    assert d.input_path == e.input_path == "relayout+interp" and _same_bits(c, d) and _same_bits(c, e)


def _blocked_inputs(dtype):
    lat, lon, hyam, hybm, ps, f, ftm, pstm, inside = _frontend(NT_BLOCKED, NLEV_BLOCKED, dtype)
    return lat, hyam, hybm, ftm, pstm, dict(plev=inside, hyam=hyam, hybm=hybm, L=30, debug_level=0, dims=TM)


def _whole(dtype):
    key = ("whole", np.dtype(dtype).name)
    if key not in _cache:
        from pytemdiags_amd import TEMDiagnostics
        lat, hyam, hybm, ftm, pstm, kw = _blocked_inputs(dtype)
        _cache[key] = TEMDiagnostics.from_model_levels(*[_dev(x) for x in ftm], lat, ps=_dev(pstm), **kw)
    return _cache[key]


def _device_fed(tb, dtype):
    key = ("blocked-dev", tb, np.dtype(dtype).name)
    if key not in _cache:
        from pytemdiags_amd import TEMDiagnostics
        lat, hyam, hybm, ftm, pstm, kw = _blocked_inputs(dtype)
        _cache[key] = TEMDiagnostics.from_model_levels(*[_dev(x) for x in ftm], lat, ps=_dev(pstm), time_block=tb, **kw)
    return _cache[key]


def _within(a, b, tol):
    from pytemdiags_amd import _lib
    for names, x, y in ((_lib.RESULT_NAMES, a._res, b._res), (_lib.ZONAL_NAMES, a._zon, b._zon)):
        for i, n in enumerate(names):
            e = fieldnorm_err(x[i].cpu().numpy(), y[i].cpu().numpy())
            assert e <= tol, (n, e)


@pytest.mark.parametrize("kind,dtype", [("ndarray", np.float64), ("memmap", np.float64), ("cpu_tensor", np.float64),
                                        ("ndarray", np.float32), ("memmap", np.float32)])
@pytest.mark.parametrize("tb", [1, 4, 11, 16])
def test_blocked_run_from_host_and_device_sources(tb, kind, dtype, tmp_path, monkeypatch):
    """NT = 24.  1 MiB ring chunks: a block of 4 snapshots of one field (2.9 MB fp64) goes up in several pieces."""
    from pytemdiags_amd import TEMDiagnostics, layout
    lat, hyam, hybm, ftm, pstm, kw = _blocked_inputs(dtype)
    monkeypatch.setattr(layout, "RING_CHUNK_BYTES", 1 << 20)
    assert 4 * NLEV_BLOCKED * lat.size * np.dtype(dtype).itemsize > 1 << 20
    dev, whole = _device_fed(tb, dtype), _whole(dtype)
    assert dev.time_block == tb and dev.block_timing is None
    if kind == "ndarray":
        src, ps = ftm, pstm
    elif kind == "cpu_tensor":
        src, ps = [torch.as_tensor(x) for x in ftm], torch.as_tensor(pstm)
    else:
        src = []
        for i, x in enumerate(ftm + [pstm]):
            m = np.memmap(str(tmp_path / ("f%d.bin" % i)), dtype=x.dtype, mode="w+", shape=x.shape)
            m[:] = x
            m.flush()
            src.append(np.memmap(str(tmp_path / ("f%d.bin" % i)), dtype=x.dtype, mode="r", shape=x.shape))
        src, ps = src[:4], src[4]
    tem = TEMDiagnostics.from_model_levels(*src, lat, ps=ps, time_block=tb, **kw)
    assert tem.input_path == "ingest"                       # a blocked host-fed run always takes the fused call
    assert _same_bits(tem, dev)                             # the device-fed blocked run of the same time_block
    tol = 1e-11 if dtype == np.float64 else 1e-5
    _within(tem, whole, tol)
    _within(dev, whole, tol)
    if tb >= NT_BLOCKED:
        assert _same_bits(tem, whole) and _same_bits(dev, whole)
    t = tem.block_timing
    nblocks = -(-NT_BLOCKED // tb)
    assert t is not None and len(t["upload_ms"]) == len(t["ingest_ms"]) == len(t["tem_ms"]) == nblocks
    assert "relayout_ms" not in t
    out = tem.vtem()
    assert isinstance(out, torch.Tensor) if kind == "cpu_tensor" else (isinstance(out, np.ndarray) and out.dtype == dtype)
    for n in ("ua", "up", "theta"):                         # native attributes are refused, as in every blocked run
        with pytest.raises(RuntimeError, match="time_block"):
            getattr(tem, n)


@pytest.mark.parametrize("tb", [NT_BLOCKED, NT_BLOCKED + 16])
def test_a_block_as_long_as_the_record_is_the_whole_run(tb):
    from pytemdiags_amd import TEMDiagnostics
    lat, hyam, hybm, ftm, pstm, kw = _blocked_inputs(np.float64)
    whole = _whole(np.float64)
    dev = TEMDiagnostics.from_model_levels(*[_dev(x) for x in ftm], lat, ps=_dev(pstm), time_block=tb, **kw)
    host = TEMDiagnostics.from_model_levels(*ftm, lat, ps=pstm, time_block=tb, **kw)
    assert _same_bits(dev, whole) and _same_bits(host, whole)
    assert len(host.block_timing["ingest_ms"]) == 1
    with pytest.raises(RuntimeError, match="time_block"):
        host.ua


def test_blocked_host_run_holds_blocks_not_the_record():
    """NT = 32 in blocks of 4, host-fed.  Peak device memory over the call, above the level at entry, stays below
    two upload slots (a model-level block of the four fields and of ps each, every array rounded up to 512 bytes) + one
    pressure-level block + the gathered results + the plan + the allocator's rounding + 1 MiB (the small tables, and
    512 bytes per small allocation).  Rounding: torch's caching allocator serves a request of 1 MiB or more from a
    block of whole 2 MiB units and hands the block out whole -- ``max_memory_allocated`` then counts all of it -- unless
    more than 1 MiB of it would be left over; so each of the five large allocations of the run (two slots, the
    pressure-level block, the gathered results and zonal intermediates) may count up to 1 MiB more than was asked for.
    The plan term is what the constructor takes, above its inputs, for one
    pressure-level block that is already on the device -- the plan with its matrices and work space and the results of
    one block --, measured here in the same way.  The bound is less than half of the bytes of the model-level record,
    which no step of the run may hold.  The library's tables exist before the measured calls."""
    from pytemdiags_amd import TEMDiagnostics, _lib, vertical
    nt, tb, dlat = 32, 4, 10
    lat, lon, hyam, hybm, ps, f, ftm, pstm, inside = _frontend(nt, NLEV_BLOCKED)
    M, nplev = 180 // dlat, inside.size
    up = lambda b: -(-b // 512) * 512
    slot = 4 * up(tb * NLEV_BLOCKED * lat.size * 8) + up(tb * lat.size * 8)
    block = 4 * lat.size * nplev * tb * 8
    results = (len(_lib.RESULT_NAMES) + len(_lib.ZONAL_NAMES)) * M * nplev * nt * 8
    slack = 1 << 20
    record = 4 * nt * NLEV_BLOCKED * lat.size * 8
    kw = dict(plev=inside, hyam=hyam, hybm=hybm, L=30, debug_level=0, dims=TM, zm_dlat=dlat, time_block=tb)
    _cache.clear()
    gc.collect()
    TEMDiagnostics.from_model_levels(*ftm, lat, ps=pstm, **kw)      # (first use: module loads, library tables)

    def peak_of(make):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        obj = make()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, obj
    g = vertical.records_to_pressure_device([_dev(x[:tb]) for x in ftm], _dev(pstm[:tb]), inside * 100.0, hyam=hyam,
                                            hybm=hybm)
    plan, one = peak_of(lambda: TEMDiagnostics(*g, lat, plev=inside, L=30, debug_level=0, zm_dlat=dlat))
    assert one._dev_fields[0].data_ptr() == g[0].data_ptr()         # its inputs were taken as they are: no copy in `plan`
    del one, g
    rounding = 5 << 20
    bound = 2 * slot + block + results + plan + rounding + slack
    assert 2 * bound < record
    peak, tem = peak_of(lambda: TEMDiagnostics.from_model_levels(*ftm, lat, ps=pstm, **kw))
    print("peak bytes above entry %d, bound %d (plan term %d), model-level record %d" % (peak, bound, plan, record))
    assert tuple(tem._res.shape) == (10, M, nplev, nt)
    assert peak <= bound
