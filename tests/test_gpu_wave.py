"""Zonal wavenumbers on the MI355X: ``TEMDiagnostics(..., lon=, wavenumbers=)``, ``sph_zonal_averager.sph_wave`` and the
C ABI of pytemdiags_amd/include/temx_wave.h against a numpy restatement of the contract written here.

Restatement.  Basis: ``scipy.special.lpmv`` with the normalisation of the header (``pbar``).  Fit: ``np.linalg.lstsq`` of
the basis on the EXPLICIT eddy of the oracle (``x - Y0 pinv(Y0) x``, ``TEMOracle.up vp thetap wapp``).  Zonal grid: the
coefficients times ``pbar`` at the output latitudes; fluxes ``(Xc Yc + Xs Ys) / 2``.  Sets: the oracle's seven zonal
means with the three fluxes replaced, through ``TEMOracle.from_zonal_means``.

Bounds: the project's own, field-normalised (``conftest.fieldnorm_err``): 1e-10 for fp64 and 2e-5 for fp32 inputs, as
in tests/test_gpu_engine.py.  The fp32 reference is the restatement of the same fp32 values widened to fp64 (the engine
widens exactly and works in fp64).  The grids have cond(Ym) < 2 (ne4 at L <= 20, ne8 at L <= 50); the two wider bases on
ne8, m = 1 at L = 60 and L = 70, have cond(Ym) = 2.5 and 3.5 (cond(Y0) = 2.3 and 3.8), checked in numpy.

Fields (``wave_fields``): the mean state of ``synth.analytic_fields`` plus, in every one of u, v, T, omega, waves 1, 2
and 4 with phases of their own, ``A_m cos(m lon + phase_m + 0.2 m t) cos^m(lat) (1 + 0.3 sin(lat))``, plus 0.1 noise:
every flux has a wave-1, a wave-2 and a wave-4 part (``analytic_fields`` itself carries wave 3 in T only and wave 4 in
u, v, omega only, so its v'theta' vanishes wave by wave)."""
import ctypes as C

import numpy as np
import pytest
import scipy.special

from conftest import fieldnorm_err
from oracle import tem_oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
TOL64, TOL32 = 1e-10, 2e-5
ZM7 = ("ub", "vb", "thetab", "wapb", "upvpb", "upwappb", "vptpb")
FLUXES = ZM7[4:]
FIELDS = ("ua", "va", "theta", "wap")
ADDITIVE = ("epfy", "epfz", "utendepfd")
_cache = {}


def _names():
    from pytemdiags_amd import _lib
    return _lib.RESULT_NAMES, _lib.ZONAL_NAMES


# ---- the restatement --------------------------------------------------------------------------------------------------
def pbar(m, L, x):
    """``Pbar_l^m(x)`` for l = m..L as ``[len(x)][L + 1 - m]``."""
    x = np.asarray(x, dtype=np.float64)
    l = np.arange(m, L + 1)
    norm = np.sqrt(2.0) * np.sqrt((2 * l + 1) / (4 * np.pi)
                                  * np.exp(scipy.special.gammaln(l - m + 1) - scipy.special.gammaln(l + m + 1)))
    return norm[None, :] * scipy.special.lpmv(m, l[None, :], x[:, None])


def wave_basis(lat, lon, m, L):
    P = pbar(m, L, np.sin(np.deg2rad(lat)))
    lam = np.deg2rad(np.asarray(lon, dtype=np.float64))[:, None]
    return np.concatenate([P * np.cos(m * lam), P * np.sin(m * lam)], axis=1)


def wave_fit(eddy, lat, lon, lat_out, m, L):
    """``eddy`` ``[N][...]`` -> (coefficients ``[Kc][D]``, Xc, Xs ``[M][...]``)."""
    e2 = np.asarray(eddy, dtype=np.float64).reshape(eddy.shape[0], -1)
    c = np.linalg.lstsq(wave_basis(lat, lon, m, L), e2, rcond=None)[0]
    n = L + 1 - m
    Pz = pbar(m, L, np.sin(np.deg2rad(lat_out)))
    shape = (len(lat_out),) + tuple(eddy.shape[1:])
    return c, (Pz @ c[:n]).reshape(shape), (Pz @ c[n:]).reshape(shape)


def wave_fields(lat, lon, plev, nt, seed=3, noise=0.1, dtype=np.float64):
    # the mean-state parts of synth.analytic_fields (its own waves left out)
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
    amps = {1: (5.0, 4.0, 2.0, 0.03), 2: (6.0, 3.0, 3.0, 0.04), 4: (8.0, 6.0, 1.5, 0.05)}
    rng = np.random.default_rng(seed)
    out = []
    for f in range(4):
        a = np.broadcast_to(zonal[f], shape).copy()
        for m, amp in amps.items():
            a += amp[f] * np.cos(m * lam + 0.9 * f + 0.4 * m + 0.2 * m * t) * c ** m * (1 + 0.3 * s)
        a += noise * rng.standard_normal(shape)
        out.append(np.ascontiguousarray(a.astype(dtype)))
    return tuple(out)


def reference(key, lat, lon, plev, fields, L, ms):
    """Computed once per key, shared, left unchanged: the oracle of the ordinary run, per m the coefficients, parts and
    fluxes, and the oracle of every set and of the residual."""
    if key in _cache:
        return _cache[key]
    f64 = [np.asarray(x, dtype=np.float64) for x in fields]
    dts = dict(ua_dtype=fields[0].dtype, va_dtype=fields[1].dtype, wap_dtype=fields[3].dtype)
    full = orc.TEMOracle(*f64, lat, plev, L=L, mode="factorised")
    eddies = (full.up, full.vp, full.thetap, full.wapp)
    ref = {"full": full, "coef": {}, "parts": {}, "flux": {}, "sets": {}}
    zm = {n: np.asarray(getattr(full, n), dtype=np.float64) for n in ZM7}
    rest = {n: zm[n].copy() for n in FLUXES}
    for m in ms:
        fit = [wave_fit(e, lat, lon, full.lat, m, L) for e in eddies]
        ref["coef"][m] = np.stack([c for c, _, _ in fit])
        ref["parts"][m] = np.stack([np.stack([xc, xs]) for _, xc, xs in fit])
        xc, xs = ref["parts"][m][:, 0], ref["parts"][m][:, 1]
        flux = {"upvpb": 0.5 * (xc[0] * xc[1] + xs[0] * xs[1]), "upwappb": 0.5 * (xc[0] * xc[3] + xs[0] * xs[3]),
                "vptpb": 0.5 * (xc[1] * xc[2] + xs[1] * xs[2])}
        ref["flux"][m] = flux
        for n in FLUXES:
            rest[n] -= flux[n]
        ref["sets"][m] = orc.TEMOracle.from_zonal_means({**zm, **flux}, full.plev, **dts)
    ref["sets"]["residual"] = orc.TEMOracle.from_zonal_means({**zm, **rest}, full.plev, **dts)
    _cache[key] = ref
    return ref


def case(kind, dtype=np.float64, desc=False):
    """(lat, lon, plev, fields, L, ms, reference) of the named shape."""
    from pytemdiags_amd import synth
    ne, nlev, nt, L, ms = {"ne4": (4, 5, 3, 12, (1, 2, 4)), "ne8": (8, 9, 5, 20, (1, 3, 20)),
                           "ne8L50": (8, 4, 2, 50, (1, 3)), "ne8L60": (8, 4, 2, 60, (1,)), "ne8L70": (8, 4, 2, 70, (1,))}[kind]
    key = (kind, np.dtype(dtype).name, desc)
    if ("case",) + key not in _cache:
        lat, lon = synth.cubed_sphere_gll(ne)
        plev = synth.pressure_levels(nlev)
        if desc:
            plev = plev[::-1].copy()
        f = wave_fields(lat, lon, plev, nt, dtype=dtype)
        for x in f:
            x.setflags(write=False)
        _cache[("case",) + key] = (lat, lon, plev, f, L, ms)
    lat, lon, plev, f, L, ms = _cache[("case",) + key]
    return lat, lon, plev, f, L, ms, reference(("ref",) + key, lat, lon, plev, f, L, ms)


def host(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def set_values(rs):
    RES, ZON = _names()
    out = {n: host(getattr(rs, n)()) for n in RES}
    out.update({n: host(getattr(rs, n)) for n in ZON})
    return out


def oracle_values(o):
    RES, ZON = _names()
    out = {n: np.asarray(getattr(o, n)(), dtype=np.float64) for n in RES}
    out.update({n: np.asarray(getattr(o, n), dtype=np.float64) for n in ZON})
    return out


def run_case(kind, dtype=np.float64, desc=False, **kw):
    from pytemdiags_amd import TEMDiagnostics
    key = ("tem", kind, np.dtype(dtype).name, desc)
    lat, lon, plev, f, L, ms, ref = case(kind, dtype, desc)
    if key not in _cache or kw:
        tem = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms, **kw)
        if kw:
            return tem, ref
        _cache[key] = tem
    return _cache[key], ref


def check_front(tem, ref, ms, tol, tag):
    """Parts, fluxes, ten results and sixteen zonal attributes of every set and of the residual, field-normalised."""
    worst = (0.0, "")
    for m in ms:
        ws = tem.waves[m]
        for i, name in enumerate(FIELDS):
            xc, xs = ws.parts(name)
            e = fieldnorm_err(np.stack([host(xc), host(xs)]), ref["parts"][m][i])
            print("%s m=%d parts(%s): %.2e" % (tag, m, name, e))
            worst = max(worst, (e, "m%d.parts.%s" % (m, name)))
        for n in FLUXES:
            e = fieldnorm_err(host(getattr(ws, n)), ref["flux"][m][n])
            print("%s m=%d flux %s: %.2e" % (tag, m, n, e))
            worst = max(worst, (e, "m%d.%s" % (m, n)))
    for s in tuple(ms) + ("residual",):
        rs = tem.waves.residual if s == "residual" else tem.waves[s]
        got, want = set_values(rs), oracle_values(ref["sets"][s])
        for n, r in want.items():
            assert got[n].shape == r.shape, (s, n, got[n].shape, r.shape)
            e = fieldnorm_err(got[n], r)
            worst = max(worst, (e, "%s.%s" % (s, n)))
    print("%s: worst field-normalised error %.2e (%s)" % (tag, worst[0], worst[1]))
    assert worst[0] <= tol, (tag, worst)


def check_coefficients(tem, ref, lon, ms, tol, tag):
    """The coefficients (and the parts again) of ua va theta wap through the operator entry point, on the engine's own
    device fields.  The operator takes a field as it is: theta's coefficients are those of ``ta`` times (p0/p)^kappa per
    level (the fit is linear), which keeps the dtype of the call that of the run."""
    from pytemdiags_amd import waves
    full = ref["full"]
    nlev, nt = tem.ua.shape[1], tem.ua.shape[2]
    th = np.repeat((full.p0 / full.p) ** orc.k, nt)                   # per column d = lev * nt + t
    th3 = th.reshape(1, 1, nlev, nt)
    st = waves.WaveState(tem.ZM._plan, lon, ms)
    try:
        for i, x in enumerate((tem.ua, tem.va, tem.ta, tem.wap)):
            for m in ms:
                parts, coef = st.project(x, m, want_coef=True)
                c, p = host(coef), host(parts)
                if i == 2:
                    c, p = c * th[None, :], p * th3
                e, ep = fieldnorm_err(c, ref["coef"][m][i]), fieldnorm_err(p, ref["parts"][m][i])
                print("%s m=%d coef(%s): %.2e  parts: %.2e" % (tag, m, FIELDS[i], e, ep))
                assert e <= tol and ep <= tol, (tag, m, FIELDS[i], e, ep)
        assert not st.status()
    finally:
        st.close()


# ---- 1-3: parity ----------------------------------------------------------------------------------------------------------
def test_parity_smallest_shape_fp64_coefficients_parts_fluxes_sets():
    """ne4 (866 columns) x 5 x 3 (D = 15), L = 12, wavenumbers (1, 2, 4).  Wave 4 is there on purpose: a fit of the raw
    fields instead of the eddies is 88 % off in its u'v'."""
    from pytemdiags_amd import waves
    tem, ref = run_case("ne4")
    lat, lon, plev, f, L, ms, _ = case("ne4")
    assert tem.waves.wavenumbers == ms and tem.waves.workspace_bytes > 0
    check_front(tem, ref, ms, TOL64, "ne4 fp64")
    check_coefficients(tem, ref, lon, ms, TOL64, "ne4 fp64")


def test_parity_fp32_inputs_typed_as_the_ordinary_run():
    tem, ref = run_case("ne4", np.float32)
    ms = tem.waves.wavenumbers
    check_front(tem, ref, ms, TOL32, "ne4 fp32")
    assert tem.ua.dtype == torch.float32
    check_coefficients(tem, ref, case("ne4", np.float32)[1], ms, TOL32, "ne4 fp32")
    ws = tem.waves[2]
    assert ws.epfy().dtype == tem.epfy().dtype == np.float32 and ws.vtem().dtype == np.float32
    assert ws.psi.dtype == tem.psi.dtype == np.float64 and ws.upvpb.dtype == tem.upvpb.dtype == np.float32
    assert ws.vptpb.dtype == np.float64
    assert ws.amplitude("ua").dtype == np.float32 and ws.amplitude("theta").dtype == np.float64
    assert tem.waves.residual.epfz().dtype == np.float32


@pytest.mark.parametrize("desc", [False, True], ids=["ascending", "descending-plev"])
def test_parity_several_d_tiles_and_splits(desc):
    """ne8 x 9 x 5 (D = 45: three d-tiles, the last with a tail), L = 20, wavenumbers (1, 3, 20): Kc = 40, 36 and, at
    m = L, a basis of two columns."""
    tem, ref = run_case("ne8", desc=desc)
    check_front(tem, ref, tem.waves.wavenumbers, TOL64, "ne8 fp64 desc=%s" % desc)


@pytest.mark.parametrize("kind,tb,nslice", [("ne8L50", 25, 1), ("ne8L60", 32, 1), ("ne8L70", 4, 2)],
                         ids=["Kc100-25-blocks", "Kc120-32-blocks", "Kc140-two-slices"])
def test_parity_wide_bases_every_instantiation_and_the_sliced_sweep(kind, tb, nslice):
    """The widths the small shapes do not reach, ne8 x 4 x 2 (D = 8): L = 50, m = 1, 3 (Kc = 100 and 96: the 25-block
    sweep of the default L, whose staging image is no multiple of the workgroup), L = 60, m = 1 (Kc = 120: 32 blocks) and
    L = 70, m = 1 (Kc = 140: a slice of 32 blocks and one of 4, the fields read twice, the reduction placed per field),
    through ``temxk_wave_fluxes`` (front end) and ``temxk_wave_project`` (coefficients)."""
    from pytemdiags_amd import _wave
    lat, lon, plev, f, L, ms, ref = case(kind)
    sh = _wave.shape(L, ms[0])
    assert (sh["tb_last"], sh["nslice"]) == (tb, nslice), sh
    tem, _ = run_case(kind)
    check_front(tem, ref, ms, TOL64, kind)
    check_coefficients(tem, ref, lon, ms, TOL64, kind)


# ---- 4: planted coefficients ----------------------------------------------------------------------------------------------
def test_planted_coefficients_come_back_with_amplitude_and_phase():
    """lat-lon 24 x 48, where cos(m lon) is exactly orthogonal to the zonal harmonics: fields built from random
    coefficients (l <= L = 10, m in 1, 2, 4) plus zonally symmetric parts from Y_l^0."""
    from pytemdiags_amd import TEMDiagnostics, synth, waves
    L, ms, nlev, nt = 10, (1, 2, 4), 3, 2
    lat, lon = synth.latlon_grid(24, 48)
    plev = synth.pressure_levels(nlev)
    rng = np.random.default_rng(17)
    Y0 = orc.ylm0_matrix(lat, L)
    D = nlev * nt
    planted, fields = {}, []
    scale = (5.0, 3.0, 2.0, 0.05)
    for f in range(4):
        a = Y0 @ (scale[f] * rng.standard_normal((L + 1, D)) / (1 + np.arange(L + 1))[:, None])
        if f == 2:
            a += 280.0
        for m in ms:
            c = scale[f] * rng.standard_normal((2 * (L + 1 - m), D))
            planted[(f, m)] = c
            a += wave_basis(lat, lon, m, L) @ c
        fields.append(np.ascontiguousarray(a.reshape(len(lat), nlev, nt)))
    tem = TEMDiagnostics(*fields, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms)
    st = waves.WaveState(tem.ZM._plan, lon, ms)
    try:
        for f, x in enumerate((tem.ua, tem.va, tem.ta, tem.wap)):
            for m in ms:
                _, coef = st.project(x, m, want_coef=True)
                e = fieldnorm_err(host(coef), planted[(f, m)])
                print("planted f=%d m=%d coef: %.2e" % (f, m, e))
                assert e <= TOL64, (f, m, e)
    finally:
        st.close()
    lat_out = tem.lat
    for m in ms:
        Pz = pbar(m, L, np.sin(np.deg2rad(lat_out)))
        n = L + 1 - m
        for f, name in ((0, "ua"), (1, "va"), (3, "wap")):     # (theta carries the factor (p0/p)^kappa per level)
            xc = (Pz @ planted[(f, m)][:n]).reshape(len(lat_out), nlev, nt)
            xs = (Pz @ planted[(f, m)][n:]).reshape(len(lat_out), nlev, nt)
            ea = fieldnorm_err(host(tem.waves[m].amplitude(name)), np.hypot(xc, xs))
            ph = np.arctan2(xs, xc) / m
            dp = np.abs(host(tem.waves[m].phase(name)) - ph)
            ep = float(np.max(np.minimum(dp, 2 * np.pi / m - dp)) / np.max(np.abs(ph)))
            print("planted m=%d %s amplitude %.2e phase %.2e" % (m, name, ea, ep))
            assert ea <= TOL64 and ep <= TOL64, (m, name, ea, ep)
    # theta: the planted T coefficients times (p0/p)^kappa
    th = (tem.p0 / (plev * 100)) ** orc.k
    for m in ms:
        Pz = pbar(m, L, np.sin(np.deg2rad(lat_out)))
        n = L + 1 - m
        c = planted[(2, m)].reshape(-1, nlev, nt) * th[None, :, None]
        xc, xs = np.tensordot(Pz, c[:n], 1), np.tensordot(Pz, c[n:], 1)
        assert fieldnorm_err(host(tem.waves[m].amplitude("theta")), np.hypot(xc, xs)) <= TOL64


# ---- 5: closure -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ne4", "ne8"])
def test_sets_plus_residual_add_up_to_the_ordinary_run(kind):
    tem, _ = run_case(kind)
    for n in ADDITIVE:
        total = host(getattr(tem, n)())
        s = host(getattr(tem.waves.residual, n)())
        for m in tem.waves.wavenumbers:
            s = s + host(getattr(tem.waves[m], n)())
        e = fieldnorm_err(s, total)
        print("%s closure %s: %.2e" % (kind, n, e))
        assert e <= TOL64, (kind, n, e)


# ---- 6: nothing else moves ------------------------------------------------------------------------------------------------
def test_ordinary_results_are_bit_identical_with_and_without_wavenumbers_and_runs_repeat():
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, L, ms, _ = case("ne4")
    plain = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0)
    with pytest.raises(RuntimeError, match="wavenumbers"):
        plain.waves
    a, _ = run_case("ne4")
    b = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms)
    va, vp, vb = set_values(a), set_values(plain), set_values(b)
    for n in va:
        assert np.array_equal(va[n], vp[n]), n
        assert np.array_equal(va[n], vb[n]), n
    for m in ms:
        wa, wb = set_values(a.waves[m]), set_values(b.waves[m])
        for n in wa:
            assert np.array_equal(wa[n], wb[n]), (m, n)
        for name in FIELDS:
            for x, y in zip(a.waves[m].parts(name), b.waves[m].parts(name)):
                assert np.array_equal(host(x), host(y)), (m, name)
    ra, rb = set_values(a.waves.residual), set_values(b.waves.residual)
    assert all(np.array_equal(ra[n], rb[n]) for n in ra)
    # tracers are unaffected
    q = np.ascontiguousarray(1e-3 * (1 + 0.1 * np.asarray(f[0]) / 30.0))
    tq = TEMDiagnostics(*f, lat, q=q, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms)
    tp = TEMDiagnostics(*f, lat, q=q, plev=plev, L=L, debug_level=0)
    assert np.array_equal(host(tq.etfy()), host(tp.etfy())) and np.array_equal(host(tq.qtendwtem()), host(tp.qtendwtem()))


# ---- 7: the operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sph_wave_against_the_restatement(dtype):
    from pytemdiags_amd import sph_zonal_averager
    lat, lon, plev, f, L, ms, ref = case("ne4")
    lat_out = orc.zm_latitudes(1)
    Z = sph_zonal_averager(lat, lat_out, L, lon=lon, debug=False)
    Z.sph_compute_matrices()
    Zo = orc.ZonalAverager(lat, lat_out, L, mode="factorised")
    tol = TOL64 if dtype == np.float64 else TOL32
    for A in (np.ascontiguousarray(f[0][:, 2, :]), np.asarray(f[1])):       # 2-D and 3-D
        A = np.ascontiguousarray(A.astype(dtype))
        A64 = A.astype(np.float64)
        for m in (1, 4):
            _, xc, xs = wave_fit(A64 - Zo.zonal_mean_native(A64), lat, lon, lat_out, m, L)
            gc, gs = Z.sph_wave(A, m)
            assert gc.dtype == dtype and gc.shape == xc.shape == (len(lat_out),) + A.shape[1:]
            e = fieldnorm_err(np.stack([gc, gs]), np.stack([xc, xs]))
            print("sph_wave %s ndim=%d m=%d: %.2e" % (np.dtype(dtype).name, A.ndim, m, e))
            assert e <= tol, (m, e)
    with pytest.raises(ValueError, match="1..L"):
        Z.sph_wave(A, L + 1)
    bad = A.copy()
    bad[7, 0] = np.nan
    with pytest.raises(RuntimeError, match="has nans"):           # temxk_wave_status, the flag of the wave state's own
        Z.sph_wave(bad, 1)
    assert not Z._plan.status()                                       # ... which the plan's temx_status does not see
    gc, _ = Z.sph_wave(A, 1)                                          # and which the call cleared
    assert np.all(np.isfinite(gc))
    Zn = sph_zonal_averager(lat, lat_out, L, debug=False)
    Zn.sph_compute_matrices()
    with pytest.raises(ValueError, match="lon="):
        Zn.sph_wave(A, 1)


# ---- 8: C ABI refusals ------------------------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_plan_usable():
    from pytemdiags_amd import _wave, engine, synth
    lib = _wave.load()
    err = lib.temx_last_error
    lat, lon = synth.cubed_sphere_gll(4)
    lat_out = orc.zm_latitudes(1)
    lon_p = np.ascontiguousarray(lon).ctypes.data_as(C.POINTER(C.c_double))

    def create(plan, ms, lon_ptr=lon_p, nm=None):
        h = C.c_void_p()
        arr = (C.c_int * max(1, len(ms)))(*ms)
        rc = lib.temxk_wave_create(C.byref(h), plan._h if plan is not None else None, lon_ptr, len(ms) if nm is None else nm, arr)
        assert (rc == 0) == bool(h.value)
        return rc, h

    plan = engine.Plan(lat, lat_out, 12, device=0)
    assert create(None, (1,))[0] == -1
    assert create(plan, (1,), lon_ptr=None)[0] == -1
    assert create(plan, (), nm=0)[0] == -1 and b"nm" in err()
    assert create(plan, (0,))[0] == -1 and b"1..L" in err()
    assert create(plan, (13,))[0] == -1 and b"1..L" in err()
    assert create(plan, (2, 3, 2))[0] == -1 and b"twice" in err()
    bad = np.array(lon)
    bad[5] = np.nan
    assert create(plan, (1,), lon_ptr=bad.ctypes.data_as(C.POINTER(C.c_double)))[0] == -1 and b"lon 5" in err()
    deferred = engine.Plan(lat, lat_out, 12, device=0, defer_finalize=True)
    assert create(deferred, (1,))[0] == -5 and b"finalised" in err()
    big = engine.Plan(lat, lat_out, 300, device=0)
    assert create(big, (1,))[0] == -6 and b"Kc = 600" in err()
    weighted = engine.Plan(lat, lat_out, 12, device=0, defer_finalize=True)
    weighted.set_weights(np.full(lat.size, 1.0 / lat.size))
    assert create(weighted, (1,))[0] == -6 and b"weights" in err()
    masked = engine.Plan(lat, lat_out, 12, device=0)
    masked.configure(missing="mask")
    assert create(masked, (1,))[0] == -6 and b"missing" in err()
    binned = engine.Plan(lat, lat_out, 12, device=0, lat_bins=True)
    assert create(binned, (1,))[0] == -6 and b"bins" in err()
    sharded = engine.Plan(lat, lat_out, 12, device=0, defer_finalize=True)
    sharded.finalize(sharded.matrix(0).T.cpu().numpy() @ sharded.matrix(0).cpu().numpy())
    assert create(sharded, (1,))[0] == -6 and b"outside" in err()
    # a good state: the calls' own refusals
    rc, h = create(plan, (1, 4))
    assert rc == 0 and lib.temxk_wave_workspace_bytes(h) > 0
    nlev, nt = 3, 2
    plev = synth.pressure_levels(nlev)
    f = [torch.as_tensor(x, device=DEV) for x in wave_fields(lat, lon, plev, nt)]
    M, D = len(lat_out), nlev * nt
    flux = torch.empty((2, 3, M, nlev, nt), dtype=torch.float64, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    fl = lambda dt=0, out=flux, u=f[0]: lib.temxk_wave_fluxes(h, ptr(u) if u is not None else None, ptr(f[1]), ptr(f[2]), ptr(f[3]), dt,
                                                              ptr(out) if out is not None else None, None, None)
    assert fl() == -5 and b"temx_plan_set_tem" in err()          # no TEM levels yet
    plan.set_tem(nlev, nt, plev * 100)
    assert fl(dt=2) == -1 and b"dtype" in err()
    assert fl(out=None) == -1 and fl(u=None) == -1
    parts = torch.empty((2, M, D), dtype=torch.float64, device=DEV)
    one, dts = (C.c_void_p * 1)(f[0].data_ptr()), (C.c_int * 1)(0)
    pj = lambda mi=0, nf=1, fields=one, dt=dts, Dv=D, out=parts: lib.temxk_wave_project(
        h, mi, nf, fields, dt, Dv, ptr(out) if out is not None else None, None, None)
    assert pj(mi=2) == -1 and b"mi" in err() and pj(mi=-1) == -1
    assert pj(nf=0) == -1 and pj(nf=9) == -1 and b"nf" in err()
    assert pj(fields=None) == -1 and pj(dt=None) == -1 and pj(out=None) == -1
    assert pj(fields=(C.c_void_p * 1)(None)) == -1
    assert pj(dt=(C.c_int * 1)(7)) == -1 and b"dtype" in err()
    assert pj(Dv=0) == -1 and b"D must" in err()
    # everything still works: the calls, and the plan's own run bit for bit as before the refusals
    assert fl() == 0 and pj() == 0
    res_a, _ = plan.tem_run(*f)
    plan.configure(missing="mask")
    assert fl() == -5                                             # (a configure asks for temx_plan_set_tem again)
    plan.set_tem(nlev, nt, plev * 100)
    assert fl() == -6 and b"missing" in err()
    plan.configure(missing="raise")
    plan.set_tem(nlev, nt, plev * 100)
    flux2 = torch.empty_like(flux)
    assert fl(out=flux2) == 0
    res_b, _ = plan.tem_run(*f)
    torch.cuda.synchronize()
    assert torch.equal(flux, flux2) and torch.equal(res_a, res_b) and not plan.status()
    lib.temxk_wave_destroy(h)
    lib.temxk_wave_destroy(None)
