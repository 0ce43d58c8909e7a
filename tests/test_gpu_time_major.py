"""Time-major records through the front end: the GPU re-layout in front of a whole run (``input_path``) and the
blocked run ``TEMDiagnostics(..., time_block=)`` from device tensors, host arrays and a memmap.

Bounds.  A blocked run against the whole run: the project's own bound between time slices and the whole run
(tests/test_gpu_sliced.py), 1e-11 for fp64 and 1e-5 for fp32, field-normalised; against the numpy oracle 1e-10 (fp64),
the bound of the smoke test.  Everything that only changes where a copy is made is compared with ``torch.equal``."""
import gc

import numpy as np
import pytest

from conftest import fieldnorm_err
from oracle import tem_oracle as orc
from test_missing_host import surface_mask

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
TM = ("time", "plev", "ncol")
NE, NLEV, NT = 10, 9, 11
_cache = {}


def _tm(x):
    """[ncol][nlev][nt] -> time-major [nt][nlev][ncol], C-contiguous."""
    return np.ascontiguousarray(np.transpose(x, (2, 1, 0)))


def _case(dtype=np.float64, nt=NT, ne=NE, nlev=NLEV):
    key = ("case", np.dtype(dtype).name, nt, ne, nlev)
    if key not in _cache:
        from pytemdiags_amd import synth
        lat, lon = synth.cubed_sphere_gll(ne)
        plev = synth.pressure_levels(nlev)
        f = synth.analytic_fields(lat, lon, plev, nt, seed=23, dtype=dtype)
        _cache[key] = (lat, lon, plev, f, [_tm(x) for x in f])
    return _cache[key]


def _whole(dtype=np.float64, **kw):
    """The whole run on the same data in engine layout: computed once, shared, left unchanged."""
    key = ("whole", np.dtype(dtype).name) + tuple(sorted(kw.items()))
    if key not in _cache:
        from pytemdiags_amd import TEMDiagnostics
        lat, lon, plev, f, _ = _case(dtype)
        _cache[key] = TEMDiagnostics(*f, lat, plev=plev, debug_level=0, **kw)
    return _cache[key]


def _same_bits(a, b):
    return torch.equal(a._res, b._res) and torch.equal(a._zon, b._zon)


def _within(a, b, tol):
    from pytemdiags_amd import _lib
    worst = 0.0
    for names, x, y in ((_lib.RESULT_NAMES, a._res, b._res), (_lib.ZONAL_NAMES, a._zon, b._zon)):
        for i, n in enumerate(names):
            e = fieldnorm_err(x[i].cpu().numpy(), y[i].cpu().numpy())
            worst = max(worst, e)
            assert e <= tol, (n, e)
    return worst


# ---- path (a): the whole run, the copy made by the re-layout ------------------------------------------------------
@pytest.mark.parametrize("variant", ["f64", "f32", "desc"])
def test_time_major_whole_run_takes_the_relayout_and_keeps_every_bit(variant, monkeypatch):
    """With the kernel switched on for whole runs (``layout.WHOLE_RUN_KERNEL``; off by default until it is measured
    against the torch copy)."""
    from pytemdiags_amd import LabeledArray, TEMDiagnostics, _lib, layout
    monkeypatch.setattr(layout, "WHOLE_RUN_KERNEL", {"float64": True, "float32": True})
    dtype = np.float32 if variant == "f32" else np.float64
    lat, lon, plev, f, ftm = _case(dtype)
    ref = _whole(dtype)
    assert ref.input_path == "torch"
    pl = plev
    if variant == "desc":                       # descending plev: the same data handed over bottom first
        ftm = [np.ascontiguousarray(x[:, ::-1, :]) for x in ftm]
        pl = plev[::-1].copy()
    kw = dict(plev=pl, dims=TM, debug_level=0)
    dev = TEMDiagnostics(*[torch.as_tensor(x, device=DEV) for x in ftm], lat, **kw)
    host = TEMDiagnostics(*ftm, lat, **kw)
    lab = TEMDiagnostics(*[LabeledArray(x, TM, {"plev": pl, "time": np.arange(NT)}, name=n)
                           for x, n in zip(ftm, ("ua", "va", "ta", "wap"))], lat, debug_level=0)
    for tem in (dev, host, lab):
        assert tem.input_path == "relayout"
        assert (tem.NCOL, tem.NLEV, tem.NT) == (lat.size, NLEV, NT) and tem.plev[0] < tem.plev[-1]
        assert _same_bits(tem, ref)
        for a, b in zip(tem._dev_fields, ref._dev_fields):
            assert a.dtype == b.dtype and torch.equal(a, b)
    # through the public getters too: kinds and dtypes as before
    for n in _lib.RESULT_NAMES:
        r = getattr(host, n)()
        assert isinstance(r, np.ndarray) and r.dtype == dtype
        np.testing.assert_array_equal(r, getattr(ref, n)())
    assert isinstance(dev.ub, torch.Tensor) and torch.equal(dev.ub, torch.as_tensor(ref.ub, device=DEV))
    assert lab.vtem().dims == ("lat", "plev", "time")
    np.testing.assert_array_equal(lab.psi.values, ref.psi)
    np.testing.assert_array_equal(host.up, ref.up)                 # native attributes exist in a whole run
    # any other order keeps the torch path, and its bits
    other = TEMDiagnostics(*[np.ascontiguousarray(np.transpose(x, (0, 2, 1))) for x in ftm], lat, plev=pl,
                           dims=("time", "ncol", "plev"), debug_level=0)
    assert other.input_path == "torch" and _same_bits(other, ref)


def test_time_major_mixed_dtypes_widen_in_the_relayout(monkeypatch):
    from pytemdiags_amd import TEMDiagnostics, layout
    monkeypatch.setattr(layout, "WHOLE_RUN_KERNEL", {"float64": True, "float32": True})
    lat, lon, plev, f, ftm = _case()
    mixed = [f[0], f[1].astype(np.float32), f[2], f[3].astype(np.float32)]
    ref = TEMDiagnostics(*mixed, lat, plev=plev, debug_level=0)
    tem = TEMDiagnostics(*[_tm(x) for x in mixed], lat, plev=plev, dims=TM, debug_level=0)
    assert tem.input_path == "relayout" and _same_bits(tem, ref)
    assert tem.vtem().dtype == np.float32 and tem.epfy().dtype == np.float64


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_whole_run_follows_the_gate_and_keeps_its_bits_either_way(dtype):
    """As committed: a time-major whole run takes the kernel exactly for the dtypes ``WHOLE_RUN_KERNEL`` switches on,
    the torch copy otherwise, with descending plev too; the results are the same bits."""
    from pytemdiags_amd import TEMDiagnostics, layout
    lat, lon, plev, f, ftm = _case(dtype)
    want = "relayout" if layout.WHOLE_RUN_KERNEL[np.dtype(dtype).name] else "torch"
    tem = TEMDiagnostics(*ftm, lat, plev=plev, dims=TM, debug_level=0)
    assert tem.input_path == want and _same_bits(tem, _whole(dtype))
    desc = [torch.as_tensor(np.ascontiguousarray(x[:, ::-1, :]), device=DEV) for x in ftm]
    tem = TEMDiagnostics(*desc, lat, plev=plev[::-1].copy(), dims=TM, debug_level=0)
    assert tem.input_path == want and _same_bits(tem, _whole(dtype))
    assert torch.equal(tem.ta, _whole(dtype).ta)
    with pytest.raises(AttributeError):
        tem.ua = None                                               # read-only: the device copies of the run


# ---- path (b): blocked runs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("tb", [1, 4, 11, 16])
def test_blocked_run_from_a_device_source(tb, dtype):
    from pytemdiags_amd import TEMDiagnostics, _lib
    lat, lon, plev, f, ftm = _case(dtype)
    ref = _whole(dtype)
    tem = TEMDiagnostics(*[torch.as_tensor(x, device=DEV) for x in ftm], lat, plev=plev, dims=TM, debug_level=0,
                         time_block=tb)
    assert tem.input_path == "relayout" and tem.time_block == tb
    assert tuple(tem._res.shape) == (10, 180, NLEV, NT) and tuple(tem._zon.shape) == (len(_lib.ZONAL_NAMES), 180, NLEV, NT)
    worst = _within(tem, ref, 1e-11 if dtype == np.float64 else 1e-5)
    print("time_block %d %s: worst field-normalised difference to the whole run %.2e" % (tb, np.dtype(dtype).name, worst))
    if tb >= NT:
        assert _same_bits(tem, ref)                                 # one block is the whole run
    if dtype == np.float64:
        if "oracle" not in _cache:
            _cache["oracle"] = orc.run_tem(*f, lat, plev, mode="factorised")
        for n in _lib.RESULT_NAMES:
            e = fieldnorm_err(getattr(tem, n)().cpu().numpy(), _cache["oracle"][n])
            assert e <= 1e-10, (n, e)
    assert isinstance(tem.ub, torch.Tensor) and tuple(tem.ub.shape) == (180, NLEV, NT)


@pytest.mark.parametrize("tb", [4, 16])
def test_blocked_run_descending_plev_and_other_orders(tb):
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, ftm = _case()
    ref = _whole()
    desc = [torch.as_tensor(np.ascontiguousarray(x[:, ::-1, :]), device=DEV) for x in ftm]
    a = TEMDiagnostics(*desc, lat, plev=plev[::-1].copy(), dims=TM, debug_level=0, time_block=tb)
    _within(a, ref, 1e-11)
    b = TEMDiagnostics(*f, lat, plev=plev, debug_level=0, time_block=tb)        # engine order: sliced by torch
    assert b.input_path == "torch"
    _within(b, ref, 1e-11)
    assert _same_bits(a, b)                                         # the same blocks, whichever way they were laid out


def _device_fed(tb, dtype):
    key = ("blocked-dev", tb, np.dtype(dtype).name)
    if key not in _cache:
        from pytemdiags_amd import TEMDiagnostics
        lat, lon, plev, f, ftm = _case(dtype)
        _cache[key] = TEMDiagnostics(*[torch.as_tensor(x, device=DEV) for x in ftm], lat, plev=plev, dims=TM,
                                     debug_level=0, time_block=tb)
    return _cache[key]


@pytest.mark.parametrize("kind,dtype", [("ndarray", np.float64), ("memmap", np.float64), ("cpu_tensor", np.float64),
                                        ("ndarray", np.float32), ("memmap", np.float32)])
@pytest.mark.parametrize("tb", [1, 4, 11, 16])
def test_blocked_run_from_a_host_source_goes_through_the_ring(tb, kind, dtype, tmp_path, monkeypatch):
    """The device-source test from host arrays: one block (one slot, no second upload), three blocks, and eleven
    (each slot reused five times, blocks smaller than a ring chunk); 1 MiB ring chunks, so a block of 4 snapshots
    (1.5 MB fp64) and a whole field (4.3 MB fp64, 2.1 MB fp32) go up in several pieces."""
    from pytemdiags_amd import TEMDiagnostics, layout
    lat, lon, plev, f, ftm = _case(dtype)
    monkeypatch.setattr(layout, "RING_CHUNK_BYTES", 1 << 20)
    assert NT * NLEV * lat.size * np.dtype(dtype).itemsize > 2 << 20
    dev = _device_fed(tb, dtype)
    if kind == "ndarray":
        src = ftm
    elif kind == "cpu_tensor":
        src = [torch.as_tensor(x) for x in ftm]
    else:
        src = []
        for i, x in enumerate(ftm):
            m = np.memmap(str(tmp_path / ("f%d.bin" % i)), dtype=x.dtype, mode="w+", shape=x.shape)
            m[:] = x
            m.flush()
            src.append(np.memmap(str(tmp_path / ("f%d.bin" % i)), dtype=x.dtype, mode="r", shape=x.shape))
    tem = TEMDiagnostics(*src, lat, plev=plev, dims=TM, debug_level=0, time_block=tb)
    assert tem.input_path == "relayout"
    assert _same_bits(tem, dev)                                     # the device-fed blocked run of the same time_block
    _within(tem, _whole(dtype), 1e-11 if dtype == np.float64 else 1e-5)
    if tb >= NT:
        assert _same_bits(tem, _whole(dtype))
    t = tem.block_timing                                            # upload, re-layout and TEM time of every block
    nblocks = -(-NT // tb)
    assert t is not None and len(t["upload_ms"]) == len(t["relayout_ms"]) == len(t["tem_ms"]) == nblocks
    out = tem.vtem()
    assert isinstance(out, torch.Tensor) if kind == "cpu_tensor" else isinstance(out, np.ndarray)
    assert out.dtype == (torch.float64 if dtype == np.float64 else torch.float32) if kind == "cpu_tensor" else out.dtype == dtype


def test_blocked_run_with_two_tracers():
    from pytemdiags_amd import TEMDiagnostics, _lib, synth
    lat, lon, plev, f, ftm = _case()
    qs = [synth.analytic_tracer(lat, lon, plev, NT, which=w) for w in (0, 1)]
    ref = TEMDiagnostics(*f, lat, q=qs, plev=plev, debug_level=0)
    for src, q in (([torch.as_tensor(x, device=DEV) for x in ftm], [torch.as_tensor(_tm(x), device=DEV) for x in qs]),
                   (ftm, [_tm(x) for x in qs])):
        tem = TEMDiagnostics(*src, lat, q=q, plev=plev, dims=TM, debug_level=0, time_block=4)
        assert tem.ntrac == 2 and tem.input_path == "relayout"
        _within(tem, ref, 1e-11)
        for qi in range(2):
            for n in _lib.TRACER_RESULT_NAMES:
                x, y = getattr(tem, n)(qi), getattr(ref, n)(qi)
                x = x.cpu().numpy() if hasattr(x, "cpu") else x
                e = fieldnorm_err(x, y)
                assert e <= 1e-11, (n, qi, e)
        for n in _lib.TRACER_ZONAL_NAMES:
            for x, y in zip(getattr(tem, n), getattr(ref, n)):
                x = x.cpu().numpy() if hasattr(x, "cpu") else x
                assert fieldnorm_err(x, y) <= 1e-11, n


def test_blocked_masked_run_matches_the_whole_masked_run():
    from pytemdiags_amd import TEMDiagnostics, _lib
    lat, lon, plev, f, _ = _case()
    miss = surface_mask(lat, lon, plev, NT)
    assert miss.any() and not miss.all()
    fm = [np.where(miss, np.nan, x) for x in f]
    ref = TEMDiagnostics(*fm, lat, plev=plev, debug_level=0, missing="mask")
    tem = TEMDiagnostics(*[torch.as_tensor(_tm(x), device=DEV) for x in fm], lat, plev=plev, dims=TM, debug_level=0,
                         missing="mask", time_block=4)

    def close(x, y, name):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        assert np.array_equal(np.isnan(x), np.isnan(y)), name        # the same NaN pattern
        ok = ~np.isnan(y)
        if ok.any():
            e = float(np.max(np.abs(x[ok] - y[ok]))) / float(np.max(np.abs(y[ok])))
            assert e <= 1e-11, (name, e)
    for i, n in enumerate(_lib.RESULT_NAMES):
        close(tem._res[i], ref._res[i], n)
    close(tem._cov, ref._cov, "coverage")
    # (the zonal intermediates share the NaN pattern; the derivatives among them, which the masked fit's conditioning
    #  reaches first, differ by up to 3.7e-11 from the whole run, dpsicoslat_dlat)
    for i, n in enumerate(_lib.ZONAL_NAMES):
        assert torch.equal(torch.isnan(tem._zon[i]), torch.isnan(ref._zon[i])), n
    assert tuple(tem.coverage.shape) == (180, NLEV, NT)


def test_nan_in_a_later_block_raises_the_reference_message():
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, ftm = _case()
    bad = [x.copy() for x in ftm]
    bad[2][NT - 1, 3, 17] = np.nan                                  # in the last block of 4 + 4 + 3
    for src in ([torch.as_tensor(x, device=DEV) for x in bad], bad):
        with pytest.raises(RuntimeError, match="Variable has nans"):
            TEMDiagnostics(*src, lat, plev=plev, dims=TM, debug_level=0, time_block=4)


def test_native_attributes_are_refused_in_a_blocked_run(tmp_path):
    from pytemdiags_amd import TEMDiagnostics, synth
    lat, lon, plev, f, ftm = _case()
    q = _tm(synth.analytic_tracer(lat, lon, plev, NT))
    tem = TEMDiagnostics(*ftm, lat, q=q, plev=plev, dims=TM, debug_level=0, time_block=4)
    for n in ("ua", "va", "ta", "wap", "theta", "up", "vp", "thetap", "wapp", "upvp", "upwapp", "vptp", "qp", "qpvp",
              "qpwapp"):
        with pytest.raises(RuntimeError, match="time_block"):
            getattr(tem, n)
    with pytest.raises(RuntimeError, match="time_block"):
        tem.iter_native()
    with pytest.raises(RuntimeError, match="time_block"):
        tem.to_netcdf(loc=str(tmp_path), include_attrs=True)
    with pytest.raises(AttributeError):
        tem.no_such_attribute
    # everything on the zonal grid works as before
    assert tem.qb[0].shape == (180, NLEV, NT) and tem.etfy().shape == (180, NLEV, NT)
    assert tem.coverage is None and set(tem.results()) == set(orc.RESULTS)
    # ... the writers included
    import scipy.io
    path = tem.to_netcdf(loc=str(tmp_path))
    with scipy.io.netcdf_file(path, "r", mmap=False) as nc:
        assert set(orc.RESULTS) <= set(nc.variables)
        np.testing.assert_array_equal(nc.variables["vtem"][:], tem.vtem())
        assert nc.variables["vtem"].shape == (180, NLEV, NT)
    qpath, = tem.q_to_netcdf(loc=str(tmp_path))
    with scipy.io.netcdf_file(qpath, "r", mmap=False) as nc:
        np.testing.assert_array_equal(nc.variables["etfy"][:], tem.etfy())


# ---- bounded memory -----------------------------------------------------------------------------------------------
def test_blocked_run_holds_one_block_not_the_record():
    """nt = 24 in blocks of 4.  Peak device memory over the constructor, above the level at entry, is at most
    (4 fields x 1 block in engine layout) + the result tensors + 1 MiB from a device source, and 3 x that block term
    (two upload buffers and one engine block) + results + 1 MiB from a host source; the whole run of the same input
    exceeds the first bound.  The cache is emptied first because ``max_memory_allocated`` counts cached blocks handed
    out larger than asked for; zm_dlat = 10 keeps the results of one block (0.13 MiB), which the 1 MiB has to hold,
    and every result tensor small."""
    from pytemdiags_amd import TEMDiagnostics, _lib
    nt, tb, dlat = 24, 4, 10
    lat, lon, plev, f, ftm = _case(nt=nt)
    M = 180 // dlat
    block = 4 * lat.size * NLEV * tb * 8
    results = (len(_lib.RESULT_NAMES) + len(_lib.ZONAL_NAMES)) * M * NLEV * nt * 8
    slack = 1 << 20
    assert (len(_lib.RESULT_NAMES) + len(_lib.ZONAL_NAMES)) * M * NLEV * tb * 8 < slack
    kw = dict(plev=plev, dims=TM, debug_level=0, zm_dlat=dlat)
    _cache.clear()
    gc.collect()
    torch.cuda.empty_cache()
    dsrc = list(torch.as_tensor(np.stack(ftm), device=DEV).unbind(0))
    TEMDiagnostics(*dsrc, lat, time_block=tb, **kw)                # (first use: module loads, library tables)

    def peak(src, **more):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        tem = TEMDiagnostics(*src, lat, **dict(kw, **more))
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        print("requested-bytes peak", torch.cuda.memory_stats().get("requested_bytes.all.peak"), "allocated at entry", base)
        assert tuple(tem._res.shape) == (10, M, NLEV, nt)
        return p
    p_dev = peak(dsrc, time_block=tb)
    p_host = peak(ftm, time_block=tb)
    p_whole = peak(dsrc)
    print("peak bytes above entry: device source %d (bound %d), host source %d (bound %d), whole run %d"
          % (p_dev, block + results + slack, p_host, 3 * block + results + slack, p_whole))
    assert p_dev <= block + results + slack
    assert p_host <= 3 * block + results + slack
    assert p_whole > block + results + slack
