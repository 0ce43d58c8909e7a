"""EP flux by time scale on the MI355X: ``TEMDiagnostics(..., time_bands=)`` against a numpy restatement written here.

Restatement.  The fields are filtered in numpy (``x_b[t] = sum_k w[k + h] x[t + k]``, fp64 accumulation, rounded to the
work dtype); ``oracle.tem_oracle.TEMOracle`` on the filtered fields gives the band's ``upvpb upwappb vptpb``; the sets are
``TEMOracle.from_zonal_means`` on (the oracle's mean state of the UNFILTERED fields at the valid times, those fluxes).

Bounds: the project's own, field-normalised (``conftest.fieldnorm_err``), as tests/test_gpu_wave.py applies them to its
sets: 1e-10 for fp64 and 2e-5 for fp32 inputs; 1e-10 for the additivity of ``epfy epfz utendepfd``; 1e-10 for the binned
case, the bound of tests/test_gpu_binned.py.

Fields (``band_fields``): the mean state of ``test_gpu_wave.wave_fields``, plus a zonal wave 1 at 0.04 cycles per step and
a zonal wave 4 at 0.3 cycles per step in every one of u, v, T, omega with phases of their own, plus 0.1 noise; ne4 (866
columns) x 3 levels x 40 times, L = 12.  Bands: ``lanczos(9, high=0.2)`` and ``lanczos(13, low=0.1)`` -- unequal lengths,
so the shorter one is padded (h = 6, 28 valid times)."""
import numpy as np
import pytest

from conftest import fieldnorm_err
from oracle import tem_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL64, TOL32, TOL_ADD, TOL_BINNED = 1e-10, 2e-5, 1e-10, 1e-10
ZM7 = ("ub", "vb", "thetab", "wapb", "upvpb", "upwappb", "vptpb")
FLUXES = ZM7[4:]
ADDITIVE = ("epfy", "epfz", "utendepfd")
NE, NLEV, NT, L = 4, 3, 40, 12
_cache = {}


def bands():
    from pytemdiags_amd.timebands import lanczos
    return {"synoptic": lanczos(9, high=0.2), "low": lanczos(13, low=0.1)}


def band_fields(lat, lon, plev, nt, seed=3, noise=0.1, dtype=np.float64):
    phi = np.deg2rad(lat)[:, None, None]
    lam = np.deg2rad(lon)[:, None, None]
    p = np.asarray(plev, dtype=np.float64)[None, :, None]
    t = np.arange(nt, dtype=np.float64)[None, None, :]
    z = -7.0 * np.log(p / 1000.0)
    s, c = np.sin(phi), np.cos(phi)
    shape = (len(lat), len(plev), nt)
    zonal = [30.0 * np.sin(2 * phi) ** 2 * np.exp(-((z - 12.0) / 8.0) ** 2) + 0.0 * t,
             0.5 * np.sin(2 * phi) + 0.0 * z + 0.0 * t,
             300.0 - 60.0 * s ** 2 - 6.5 * np.minimum(z, 12.0) + 2.0 * np.maximum(z - 20.0, 0.0) + 0.0 * t,
             0.01 * np.cos(3 * phi) + 0.0 * z + 0.0 * t]
    waves = {1: ((5.0, 4.0, 2.0, 0.03), 0.04), 4: ((8.0, 6.0, 1.5, 0.05), 0.3)}      # m: (amplitudes, cycles per step)
    rng = np.random.default_rng(seed)
    out = []
    for f in range(4):
        a = np.broadcast_to(zonal[f], shape).copy()
        for m, (amp, freq) in waves.items():
            a += amp[f] * np.cos(m * lam + 0.9 * f + 0.4 * m + 2 * np.pi * freq * t) * c ** m * (1 + 0.3 * s)
        a += noise * rng.standard_normal(shape)
        out.append(np.ascontiguousarray(a.astype(dtype)))
    return tuple(out)


def np_filter(x, w, dtype):
    """``x`` ``[..][nt]`` -> ``[..][nt - nw + 1]``: fp64 accumulation, rounded to ``dtype``."""
    win = np.lib.stride_tricks.sliding_window_view(np.asarray(x, dtype=np.float64), w.size, axis=-1)
    return np.ascontiguousarray((win @ w).astype(dtype))


def case(dtype=np.float64):
    """(lat, lon, plev, fields, padded weights by name, h, reference): built once per dtype, shared, left unchanged."""
    from pytemdiags_amd import synth, timebands
    key = np.dtype(dtype).name
    if key not in _cache:
        lat, lon = synth.cubed_sphere_gll(NE)
        plev = synth.pressure_levels(NLEV)
        f = band_fields(lat, lon, plev, NT, dtype=dtype)
        for x in f:
            x.setflags(write=False)
        names, table, h = timebands.check_bands(bands())
        assert names == ("synoptic", "low") and h == 6 and table.shape == (2, 13) and table[0, 0] == table[0, 1] == 0.0
        f64 = [np.asarray(x, dtype=np.float64) for x in f]
        dts = dict(ua_dtype=f[0].dtype, va_dtype=f[1].dtype, wap_dtype=f[3].dtype)
        full = orc.TEMOracle(*f64, lat, plev, L=L, mode="factorised")
        zm = {n: np.asarray(getattr(full, n), dtype=np.float64)[..., h:NT - h] for n in ZM7}
        ref = {"full": full, "zm": zm, "flux": {}, "sets": {}, "mean": {}, "dts": dts}
        rest = {n: zm[n].copy() for n in FLUXES}
        for b, name in enumerate(names):
            filt = [np_filter(x, table[b], dtype).astype(np.float64) for x in f64]
            o = orc.TEMOracle(*filt, lat, plev, L=L, mode="factorised")
            flux = {n: np.asarray(getattr(o, n), dtype=np.float64) for n in FLUXES}
            ref["flux"][name] = flux
            for n in FLUXES:
                rest[n] -= flux[n]
        ref["flux"]["residual"] = rest
        for name, flux in ref["flux"].items():
            ref["sets"][name] = orc.TEMOracle.from_zonal_means({**zm, **flux}, full.plev, **dts)
            mean = {n: v.mean(axis=-1, keepdims=True) for n, v in {**zm, **flux}.items()}
            ref["mean"][name] = orc.TEMOracle.from_zonal_means(mean, full.plev, **dts)
        _cache[key] = (lat, lon, plev, f, dict(zip(names, table)), h, ref)
    return _cache[key]


def build(dtype=np.float64, **kw):
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, _, _, _ = case(dtype)
    return TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, **kw)


def tem_of(dtype=np.float64):
    key = ("tem", np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = build(dtype, time_bands=bands())
    return _cache[key]


def host(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def names():
    from pytemdiags_amd import _lib
    return _lib.RESULT_NAMES, _lib.ZONAL_NAMES


def set_values(rs):
    RES, ZON = names()
    out = {n: host(getattr(rs, n)()) for n in RES}
    out.update({n: host(getattr(rs, n)) for n in ZON})
    return out


def oracle_values(o):
    RES, ZON = names()
    out = {n: np.asarray(getattr(o, n)(), dtype=np.float64) for n in RES}
    out.update({n: np.asarray(getattr(o, n), dtype=np.float64) for n in ZON})
    return out


def check_sets(bandsobj, refsets, nts, tol, tag):
    worst = (0.0, "")
    for s in tuple(bandsobj.names) + ("residual",):
        rs = bandsobj.residual if s == "residual" else bandsobj[s]
        got, want = set_values(rs), oracle_values(refsets[s])
        assert len(got) == 26
        for n, r in want.items():
            assert got[n].shape == r.shape == (180, NLEV, nts), (s, n, got[n].shape, r.shape)
            e = fieldnorm_err(got[n], r)
            worst = max(worst, (e, "%s.%s" % (s, n)))
    print("%s: worst field-normalised error %.2e (%s)" % (tag, worst[0], worst[1]))
    assert worst[0] <= tol, (tag, worst)


# ---- parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(np.float64, TOL64), (np.float32, TOL32)], ids=["fp64", "fp32"])
def test_band_fluxes_and_sets_against_the_restatement(dtype, tol):
    """Measured on the MI355X: band fluxes 1.2e-14 (fp64) and 4.3e-8 (fp32) at worst; the 26 quantities of every set
    7.1e-13 (fp64, residual.dpsicoslat_dlat) and 3.7e-7 (fp32, low.epdiv)."""
    tem = tem_of(dtype)
    _, _, _, f, table, h, ref = case(dtype)
    tb = tem.bands
    assert tb.names == ("synoptic", "low") and tb.half_width == h == 6 and tb.filter_path == "kernel" and len(tb) == 2
    assert np.array_equal(tb.weights, np.stack([table[n] for n in tb.names]))
    ntv = NT - 2 * h
    assert tb.workspace_bytes == 2 * 4 * f[0].shape[0] * NLEV * ntv * f[0].itemsize + 2 * 13 * 8
    assert np.array_equal(tb.time, np.arange(NT)[h:NT - h])
    worst = (0.0, "")
    for name in tb.names:
        for n in FLUXES:
            e = fieldnorm_err(host(getattr(tb[name], n)), ref["flux"][name][n])
            print("%s %s flux %s: %.2e" % (np.dtype(dtype).name, name, n, e))
            worst = max(worst, (e, name + "." + n))
        # the mean state of every set is the ordinary run's at the valid times, bit for bit
        for n, src in (("ub", tem.ub), ("vb", tem.vb), ("thetab", tem.thetab), ("wapb", tem.wapb)):
            assert np.array_equal(host(getattr(tb[name], n)), host(src)[..., h:NT - h]), (name, n)
    assert worst[0] <= tol, worst
    check_sets(tb, ref["sets"], ntv, tol, "%s sets" % np.dtype(dtype).name)
    # the bands do what their names say: wave 4 (0.3 cycles per step) is synoptic, wave 1 (0.04) is low
    big = {name: float(np.max(np.abs(ref["flux"][name]["upvpb"]))) for name in tb.names}
    assert min(big.values()) > 1.0
    with pytest.raises(KeyError, match="was not requested"):
        tb["monthly"]
    if dtype == np.float32:
        assert tb["low"].epfy().dtype == tem.epfy().dtype == np.float32 and tb["low"].psi.dtype == np.float64
        assert tem.ua.dtype == torch.float32


def test_bands_plus_residual_add_up_to_the_ordinary_run():
    tem = tem_of()
    h = tem.bands.half_width
    for n in ADDITIVE:
        total = host(getattr(tem, n)())[..., h:NT - h]
        s = host(getattr(tem.bands.residual, n)())
        for name in tem.bands:
            s = s + host(getattr(tem.bands[name], n)())
        e = fieldnorm_err(s, total)
        print("additivity %s: %.2e" % (n, e))
        assert e <= TOL_ADD, (n, e)


def test_time_mean_against_the_restatement_on_the_time_means():
    tem = tem_of()
    _, _, _, _, _, h, ref = case()
    tm = tem.bands.time_mean()
    assert tm.names == tem.bands.names and tm.time_mean() is tm and tem.bands.time_mean() is tm
    assert np.allclose(tm.time, [np.arange(NT)[h:NT - h].mean()])
    check_sets(tm, ref["mean"], 1, TOL64, "time_mean")


def test_ordinary_results_tracers_and_native_eddies_are_bit_identical_and_runs_repeat():
    lat, lon, plev, f, _, _, _ = case()
    plain = build()
    with pytest.raises(RuntimeError, match="time_bands"):
        plain.bands
    a, b = tem_of(), build(time_bands=bands())
    va, vp, vb = set_values(a), set_values(plain), set_values(b)
    for n in va:
        assert np.array_equal(va[n], vp[n]), n
        assert np.array_equal(va[n], vb[n]), n
    assert np.array_equal(host(a.up), host(plain.up)) and np.array_equal(host(a.vptp), host(plain.vptp))
    for s in a.bands.names + ("residual",):
        ra = set_values(a.bands.residual if s == "residual" else a.bands[s])
        rb = set_values(b.bands.residual if s == "residual" else b.bands[s])
        assert all(np.array_equal(ra[n], rb[n]) for n in ra), s
    q = np.ascontiguousarray(1e-3 * (1 + 0.1 * np.asarray(f[0]) / 30.0))
    tq, tp = build(q=q, time_bands=bands()), build(q=q)
    assert np.array_equal(host(tq.etfy()), host(tp.etfy())) and np.array_equal(host(tq.qtendwtem()), host(tp.qtendwtem()))
    assert np.array_equal(host(tq.qp[0]), host(tp.qp[0]))
    assert np.array_equal(host(tq.bands["low"].epfy()), host(a.bands["low"].epfy()))


def test_one_band_through_from_model_levels_equals_the_constructor():
    """``from_model_levels`` passes the keyword through: fields that already lie on the target levels (``p_model``
    equal to them) come out as the constructor's."""
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, table, h, ref = case()
    one = {"low": bands()["low"]}
    pm = np.ascontiguousarray(np.broadcast_to((plev * 100.0)[None, :, None], f[0].shape))
    a = TEMDiagnostics.from_model_levels(*f, lat, plev=plev, p_model=pm, interp="linear", edge="hold", L=L, debug_level=0, time_bands=one)
    assert a.bands.names == ("low",) and a.bands.half_width == 6
    for n in FLUXES:
        assert fieldnorm_err(host(getattr(a.bands["low"], n)), ref["flux"]["low"][n]) <= TOL64, n


def test_latitude_bins_run_the_band_sets_too():
    tem = build(time_bands=bands(), lat_bins=True)
    _, _, _, _, _, h, ref = case()
    assert tem.sweep_form == "binned"
    check_sets(tem.bands, ref["sets"], NT - 2 * h, TOL_BINNED, "lat_bins=True")
