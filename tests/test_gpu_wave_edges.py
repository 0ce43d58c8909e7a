"""The zonal-wavenumber fit on the MI355X where tests/test_gpu_wave.py does not reach: launch blocks beyond the first,
fp32 inputs on the wide instantiations, long chunk ranges per split, one split with a ragged last chunk, three slices,
the rank refusal of ``temxk_wave_create``, the confinement of a non-finite value, workspace growth and reuse on a side
stream, guards around the outputs, and longitudes given in other conventions.

The restatement is that of tests/test_gpu_wave.py, imported (``pbar``, ``wave_basis``, ``wave_fit``, ``wave_fields``,
``reference``, ``check_front``, ``check_coefficients``, ``host``).  The big-D cases and the three-slice case keep the
oracle out: the reference is ``wave_fit`` of the explicit eddy ``x - ZonalAverager.zonal_mean_native(x)``, on
``waves.WaveState`` directly.

Bounds: the project's own, field-normalised (``conftest.fieldnorm_err``): ``TOL64 = 1e-10`` for fp64 and ``TOL32 = 2e-5``
for fp32 inputs; the fp32 reference is the restatement of the same fp32 values widened to fp64.  "Bitwise" is
``torch.equal``.  No test asserts a split count (``choose_split`` depends on the CU count) except where the count holds on
any device: 7 chunks can be cut only once (``nchunk / minchunk = 1``).

Conditioning (numpy): ne4 at L = 12 and ne8 at L <= 50 cond(Ym) < 2; ne8, m = 1 at L = 60 / 70 cond(Ym) = 2.5 / 3.5; ne16,
m = 1 at L = 130 cond(Ym) = 2.6 (cond(Y0) = 3.1; m = 2 there has 5.9 and is not used); lat-lon 6 x 17 at L = 4 cond(Ym) <=
1.43 (cond(Y0) = 2.2); 12 x 16 at L = 8: m = 7 cond 1.03, m = 8 (Nyquist) 8.6e14; 32 x 48 at L = 24: m = 23 cond 1.01,
m = 24 1.5e14.

Measured worst errors (MI355X, 256 CUs; every case prints its own):
  1  ne4 D = 259 front end and operator     fp64 6.5e-13 (residual.dpsicoslat_dlat)   fp32 2.3e-07 (a set's utendepfd)
  2  guards                                  untouched; the inside differs from the exact-size call by 0 (fp64 and fp32)
  3  fp32 on the wide instantiations         L = 50: 1.8e-07   L = 60: 1.8e-07   L = 70 (two slices): 1.2e-07
  4  ne8 D = 2054, parts / fluxes / coef     L = 50 fp64 3.3e-13   L = 60 fp64 6.0e-13   L = 60 fp32 5.4e-13 (parts of
     theta each time; the coefficients of ua 2.1e-15 .. 3.3e-15)
  5  6 x 17, one split                       D = 15: fp64 4.0e-13, fp32 3.8e-07   D = 259: fp64 4.0e-13, fp32 1.5e-07
  6  ne16 L = 130, three slices              coef 9.4e-16 (per slice 7.5e-16, 9.4e-16, 4.0e-16), parts 1.4e-14
  7  12 x 16 L = 8 planted                   m = 1 coef 1.3e-14, m = 7 coef 6.9e-15; sph_wave m = 7 3.1e-14
  10 longitudes                              [-180, 180) 9.6e-16, + 720 3.1e-15; + 37: amplitude 1.1e-15, phase 2.5e-15
     (m = 4 leaves out 9.8 % of the points, m = 1 none)
Tests 8 and 9 are bitwise throughout.
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_wave as w
from conftest import fieldnorm_err
from oracle import tem_oracle as orc
from test_gpu_wave import FIELDS, FLUXES, TOL32, TOL64, host

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = -7.25e300
PAD = 4096                       # doubles of guard in front of and behind every output
MS = (1, 2, 4)
_cache = {}


def _tol(dtype):
    return TOL64 if np.dtype(dtype) == np.float64 else TOL32


def _dev(fields):
    return [torch.tensor(x, device=DEV) for x in fields]            # (a copy: the cached fields are read-only)


def shape_case(grid, nlev, nt, L, ms, dtype):
    """(lat, lon, plev, fields, reference) of a grid ("ne4" or (nlat, nlon)) x nlev x nt at truncation L: the fields
    and the reference of tests/test_gpu_wave.py (oracle of the ordinary run, per m coefficients, parts, fluxes, sets),
    computed once per key and left unchanged."""
    from pytemdiags_amd import synth
    key = (grid, nlev, nt, L, tuple(ms), np.dtype(dtype).name)
    if key not in _cache:
        lat, lon = synth.cubed_sphere_gll(int(grid[2:])) if isinstance(grid, str) else synth.latlon_grid(*grid)
        plev = synth.pressure_levels(nlev)
        f = w.wave_fields(lat, lon, plev, nt, dtype=dtype)
        for x in f:
            x.setflags(write=False)
        _cache[key] = (lat, lon, plev, f, w.reference(("edges",) + key, lat, lon, plev, f, L, ms))
    return _cache[key]


def front(grid, nlev, nt, L, ms, dtype, tag):
    """``TEMDiagnostics`` (parts, fluxes, sets, residual) and the operator (coefficients, parts) of one shape."""
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, ref = shape_case(grid, nlev, nt, L, ms, dtype)
    tem = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms)
    assert tem.waves.wavenumbers == tuple(ms) and tem.ua.dtype == (torch.float64 if dtype == np.float64 else torch.float32)
    w.check_front(tem, ref, ms, _tol(dtype), tag)
    w.check_coefficients(tem, ref, lon, ms, _tol(dtype), tag)


def eddy_fit(lat, lon, lat_out, L, m, x64, Zo=None):
    """``wave_fit`` of the explicit eddy of one fp64 field ``[N][...]`` -> (coef [Kc][D], Xc, Xs [M][...])."""
    Zo = Zo or orc.ZonalAverager(lat, lat_out, L, mode="factorised")
    return w.wave_fit(x64 - Zo.zonal_mean_native(x64), lat, lon, lat_out, m, L)


def fluxes_of(parts):
    """parts [4][2][...] (Xc, Xs of ua va theta wap) -> the three fluxes in the order of ``FLUXES``."""
    xc, xs = parts[:, 0], parts[:, 1]
    return np.stack([0.5 * (xc[0] * xc[1] + xs[0] * xs[1]), 0.5 * (xc[0] * xc[3] + xs[0] * xs[3]),
                     0.5 * (xc[1] * xc[2] + xs[1] * xs[2])])


# ---- 1: columns beyond one launch block -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_columns_beyond_one_launch_block(dtype):
    """ne4 x 7 x 37 (D = 259), L = 12, wavenumbers (1, 2, 4): 17 d-tiles, the last with 3 columns; ``wave_solve_kernel``
    runs five blocks along d, the last with 3 live columns; ``wave_parts_kernel`` and ``wave_flux_kernel`` get a second
    block with 3 live threads; the one-field sweep gets a ragged workgroup (17 = 4 * 4 + 1 d-tiles)."""
    front("ne4", 7, 37, 12, MS, dtype, "ne4 D=259 %s" % np.dtype(dtype).name)


# ---- 2: nothing written outside the outputs -----------------------------------------------------------------------------------
def _guarded(n):
    big = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float64, device=DEV)
    return big, big[PAD:PAD + n]


def _guards_untouched(big, n):
    want = torch.full((PAD,), CANARY, dtype=torch.float64, device=DEV)
    return torch.equal(big[:PAD], want) and torch.equal(big[PAD + n:], want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_nothing_is_written_outside_the_outputs(dtype):
    """The shape of test 1 through the C ABI, every output inside a larger tensor of canaries with 4096 doubles in front
    and behind: ``temxk_wave_fluxes`` with parts and ``temxk_wave_project`` with coefficients leave the guards bitwise
    untouched, overwrite every entry inside, and the inside is that of ``WaveState.fluxes`` / ``WaveState.project`` (the
    call path of test 1) within the bound."""
    from pytemdiags_amd import _lib, engine, waves
    lat, lon, plev, f, _ = shape_case("ne4", 7, 37, 12, MS, dtype)
    nlev, nt = 7, 37
    D, tol = nlev * nt, _tol(dtype)
    lat_out = orc.zm_latitudes(1)
    M = len(lat_out)
    plan = engine.Plan(lat, lat_out, 12, device=0)
    plan.set_tem(nlev, nt, plev * 100, p0=orc.P0)
    dev = _dev(f)
    dt = engine._DT[dev[0].dtype]
    st = waves.WaveState(plan, lon, MS)
    lib = st.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    try:
        flux_ref, parts_ref = st.fluxes(*dev, want_parts=True)
        nfl, npt = len(MS) * 3 * M * D, len(MS) * 8 * M * D
        bf, flux = _guarded(nfl)
        bp, parts = _guarded(npt)
        _lib.check(lib.temxk_wave_fluxes(st._h, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), dt, ptr(flux), ptr(parts), None))
        torch.cuda.synchronize()
        assert _guards_untouched(bf, nfl) and _guards_untouched(bp, npt)
        assert bool((flux != CANARY).all()) and bool((parts != CANARY).all())
        worst = 0.0
        for i in range(len(MS)):
            for j in range(3):
                worst = max(worst, fieldnorm_err(host(flux.view(len(MS), 3, -1)[i, j]), host(flux_ref[i, j]).ravel()))
            for j in range(4):
                worst = max(worst, fieldnorm_err(host(parts.view(len(MS), 4, -1)[i, j]), host(parts_ref[i, j]).ravel()))
        for mi, m in enumerate(MS):
            Kc = 2 * (12 + 1 - m)
            p_ref, c_ref = st.project(dev[3], m, want_coef=True)
            bq, pj = _guarded(2 * M * D)
            bc, coef = _guarded(Kc * D)
            one, dts = (C.c_void_p * 1)(dev[3].data_ptr()), (C.c_int * 1)(dt)
            _lib.check(lib.temxk_wave_project(st._h, mi, 1, one, dts, D, ptr(pj), ptr(coef), None))
            torch.cuda.synchronize()
            assert _guards_untouched(bq, 2 * M * D) and _guards_untouched(bc, Kc * D), m
            assert bool((pj != CANARY).all()) and bool((coef != CANARY).all()), m
            worst = max(worst, fieldnorm_err(host(pj), host(p_ref).ravel()), fieldnorm_err(host(coef), host(c_ref).ravel()))
        assert not st.status()
        print("guards %s: untouched; worst difference from the exact-size call %.2e" % (np.dtype(dtype).name, worst))
        assert worst <= tol, worst
    finally:
        st.close()
        plan.close()


# ---- 3: fp32 inputs on the wide instantiations ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tb,nslice", [("ne8L50", 25, 1), ("ne8L60", 32, 1), ("ne8L70", 4, 2)],
                         ids=["Kc100-25-blocks", "Kc120-32-blocks", "Kc140-two-slices"])
def test_fp32_inputs_on_the_wide_instantiations(kind, tb, nslice):
    """The three wide cases of tests/test_gpu_wave.py (ne8 x 4 x 2; L = 50, m = 1, 3; L = 60, m = 1; L = 70, m = 1) with
    fp32 fields: ``project_kernel<float, NF, 1, 25 or 32, 2, 2>`` and the two-slice sweep, for NF = 4 (front end) and
    NF = 1 (operator)."""
    from pytemdiags_amd import _wave
    lat, lon, plev, f, L, ms, ref = w.case(kind, np.float32)
    sh = _wave.shape(L, ms[0])
    assert (sh["tb_last"], sh["nslice"]) == (tb, nslice), sh
    tem, _ = w.run_case(kind, np.float32)
    assert tem.ua.dtype == torch.float32
    w.check_front(tem, ref, ms, TOL32, kind + " fp32")
    w.check_coefficients(tem, ref, lon, ms, TOL32, kind + " fp32")


# ---- 4: long chunk ranges ---------------------------------------------------------------------------------------------------------
class TestLongChunkRanges:
    """ne8 (3458 columns, 217 chunks) x 13 x 158 (D = 2054: 129 d-tiles, the last with 6 columns), m = 1 at L = 50 (25
    blocks, fp64) and L = 60 (32 blocks, fp64 and fp32).  On 256 CUs the four-field sweep is cut into about 15 splits of 14
    or 15 chunks and the one-field sweep into about 31 of 7 (tests/test_gpu_wave.py reaches 4 chunks per split): the
    clamp-free steady-state loop, ring slots reused over many groups.  ``WaveState.fluxes`` with parts after
    ``plan.set_tem`` and ``WaveState.project`` of ``ua`` with coefficients, against ``wave_fit`` of the explicit eddy.
    The four fp64 fields (227 MB) are built once for the class and freed with it."""
    NLEV, NT = 13, 158

    @pytest.fixture(scope="class")
    def big(self):
        from pytemdiags_amd import synth
        lat, lon = synth.cubed_sphere_gll(8)
        plev = synth.pressure_levels(self.NLEV)
        hold = {"grid": (lat, lon, plev), "f64": w.wave_fields(lat, lon, plev, self.NT)}
        yield hold
        hold.clear()
        torch.cuda.empty_cache()

    @pytest.mark.parametrize("L,dtype", [(50, np.float64), (60, np.float64), (60, np.float32)],
                             ids=["L50-25-blocks-fp64", "L60-32-blocks-fp64", "L60-32-blocks-fp32"])
    def test_long_chunk_ranges(self, big, L, dtype):
        from pytemdiags_amd import engine, waves
        lat, lon, plev = big["grid"]
        nlev, nt, m = self.NLEV, self.NT, 1
        assert lat.size == 3458 and (nlev * nt + 15) // 16 == 129 and nlev * nt % 16 == 6
        f = big["f64"] if dtype == np.float64 else tuple(x.astype(np.float32) for x in big["f64"])
        lat_out = orc.zm_latitudes(1)
        tol, tag = _tol(dtype), "ne8 D=2054 L=%d %s" % (L, np.dtype(dtype).name)
        plan = engine.Plan(lat, lat_out, L, device=0)
        plan.set_tem(nlev, nt, plev * 100, p0=orc.P0)
        dev = _dev(f)
        st = waves.WaveState(plan, lon, (m,))
        try:
            flux, parts = st.fluxes(*dev, want_parts=True)
            pj, coef = st.project(dev[0], m, want_coef=True)
            assert not st.status()
            flux, parts, pj, coef = host(flux)[0], host(parts)[0], host(pj), host(coef)
        finally:
            st.close()
            plan.close()
            del dev
            torch.cuda.empty_cache()
        # the restatement, all four fields in one fit: theta = T (p0/p)^kappa per level, fp32 values widened exactly
        if ("Zo", L) not in big:
            big[("Zo", L)] = orc.ZonalAverager(lat, lat_out, L, mode="factorised")
        th = ((orc.P0 / (plev * 100)) ** orc.k)[None, :, None]
        x64 = np.stack([np.asarray(x, dtype=np.float64) * (th if i == 2 else 1.0) for i, x in enumerate(f)], axis=1)
        c, xc, xs = eddy_fit(lat, lon, lat_out, L, m, x64, big[("Zo", L)])     # [Kc][4 D], [M][4][nlev][nt]
        del x64
        c = c.reshape(c.shape[0], 4, nlev * nt)
        want = np.stack([xc, xs]).transpose(2, 0, 1, 3, 4)                      # [4][2][M][nlev][nt]
        worst = (0.0, "")
        for i in range(4):
            e = fieldnorm_err(parts[i], want[i])
            print("%s parts(%s): %.2e" % (tag, FIELDS[i], e))
            worst = max(worst, (e, "parts." + FIELDS[i]))
        e, ep = fieldnorm_err(coef, c[:, 0]), fieldnorm_err(pj, want[0])
        print("%s project(ua): coef %.2e parts %.2e" % (tag, e, ep))
        worst = max(worst, (e, "coef.ua"), (ep, "project.parts.ua"))
        for j, r in enumerate(fluxes_of(want)):
            e = fieldnorm_err(flux[j], r)
            print("%s flux %s: %.2e" % (tag, FLUXES[j], e))
            worst = max(worst, (e, FLUXES[j]))
        print("%s: worst field-normalised error %.2e (%s)" % (tag, worst[0], worst[1]))
        assert worst[0] <= tol, (tag, worst)


# ---- 5: one split, ragged last chunk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nlev,nt", [(5, 3), (7, 37)], ids=["D15", "D259"])
def test_one_split_and_a_ragged_last_chunk(nlev, nt, dtype):
    """lat-lon 6 x 17: 102 columns, 7 chunks, which ``choose_split`` can cut only once on any device (``nsplit == 1``:
    the reduction is a copy plus the flag); the last chunk has one full group, one group with 2 rows and two empty
    groups.  L = 4, wavenumbers (1, 2, 4) (Kc = 8, 6, 2), D = 15 and D = 259, front end and operator."""
    from pytemdiags_amd import synth
    lat, _ = synth.latlon_grid(6, 17)
    assert lat.size == 102 and (lat.size + 15) // 16 == 7 and lat.size % 16 == 6
    front((6, 17), nlev, nt, 4, MS, dtype, "6x17 D=%d %s" % (nlev * nt, np.dtype(dtype).name))


# ---- 6: three slices ----------------------------------------------------------------------------------------------------------------
def test_three_slices_a_middle_slice_followed_by_another():
    """ne16 (13826 columns), L = 130, m = 1: Kc = 260 is 65 blocks, slices of 32, 32 and 1 block (the last in the 4-block
    instantiation; the second starts at block 32, the third at block 64).  D = 8, fp64, the operator with coefficients."""
    from pytemdiags_amd import _wave, engine, synth, waves
    L, m, nlev, nt = 130, 1, 4, 2
    sh = _wave.shape(L, m)
    assert sh == dict(ndeg=130, Kc=260, nslice=3, tb_last=4, gstride=68, kpad=272), sh
    lat, lon = synth.cubed_sphere_gll(16)
    assert lat.size == 13826
    plev = synth.pressure_levels(nlev)
    ua = w.wave_fields(lat, lon, plev, nt)[0]
    lat_out = orc.zm_latitudes(1)
    plan = engine.Plan(lat, lat_out, L, device=0)
    st = waves.WaveState(plan, lon, (m,))
    try:
        parts, coef = st.project(torch.as_tensor(ua, device=DEV), m, want_coef=True)
        assert not st.status()
        parts, coef = host(parts), host(coef)
    finally:
        st.close()
        plan.close()
    c, xc, xs = eddy_fit(lat, lon, lat_out, L, m, ua)
    e, ep = fieldnorm_err(coef, c), fieldnorm_err(parts, np.stack([xc, xs]))
    per_slice = [float(np.max(np.abs(coef[a:b] - c[a:b])) / np.max(np.abs(c))) for a, b in ((0, 128), (128, 256), (256, 260))]
    print("ne16 L=130 m=1 three slices: coef %.2e (slices %s) parts %.2e" % (e, " ".join("%.2e" % v for v in per_slice), ep))
    assert e <= TOL64 and ep <= TOL64, (e, ep, per_slice)


# ---- 7: rank refusal ------------------------------------------------------------------------------------------------------------------
def _create(lib, plan, lon, ms):
    h = C.c_void_p()
    lon = np.ascontiguousarray(lon, dtype=np.float64)
    rc = lib.temxk_wave_create(C.byref(h), plan._h, lon.ctypes.data_as(C.POINTER(C.c_double)), len(ms), (C.c_int * len(ms))(*ms))
    return rc, h


def test_rank_refusal_at_the_nyquist_wavenumber():
    """lat-lon 12 x 16 at L = 8: sin(8 lon) is 1e-16 at every column, cond(Ym) = 8.6e14, the Gram diagonal 2.8e-29 beside
    20.0.  ``temxk_wave_create`` refuses (8,) and (1, 8) with ``TEMX_ERANK`` and m = 8, Kc and the pivot in the message,
    the handle stays null, and the plan's ``tem_run`` is bitwise what it was; (1, 7) is accepted (cond 1.03) and planted
    coefficients of m = 1 and m = 7 come back.  The same through ``TEMDiagnostics`` and ``sph_wave``.  The bare refusal again on
    32 x 48 at L = 24: m = 24 refused, m = 23 accepted."""
    from pytemdiags_amd import TEMDiagnostics, _lib, _wave, engine, sph_zonal_averager, synth
    lib = _wave.load()
    err = lib.temx_last_error
    L, nlev, nt = 8, 3, 2
    D = nlev * nt
    lat, lon = synth.latlon_grid(12, 16)
    assert lat.size == 192
    lat_out = orc.zm_latitudes(1)
    plev = synth.pressure_levels(nlev)
    fnp = w.wave_fields(lat, lon, plev, nt)
    f = _dev(fnp)
    plan = engine.Plan(lat, lat_out, L, device=0)
    plan.set_tem(nlev, nt, plev * 100)
    res_a, _ = plan.tem_run(*f)
    assert not plan.status()
    for ms in ((8,), (1, 8)):
        rc, h = _create(lib, plan, lon, ms)
        msg = err()
        assert rc == -4 and not h.value, (ms, rc, msg)
        assert b"m = 8" in msg and b"2 basis columns" in msg and b"(pivot 1)" in msg and b"L = 8" in msg, msg
    res_b, _ = plan.tem_run(*f)
    assert not plan.status()
    torch.cuda.synchronize()
    assert torch.equal(res_a, res_b)
    # the neighbour is accepted, and fits: planted coefficients of m = 1 and m = 7 on top of a zonally symmetric part
    rc, h = _create(lib, plan, lon, (1, 7))
    assert rc == 0 and h.value, err()
    try:
        rng = np.random.default_rng(29)
        a = 280.0 + orc.ylm0_matrix(lat, L) @ (3.0 * rng.standard_normal((L + 1, D)) / (1 + np.arange(L + 1))[:, None])
        planted = {}
        for m in (1, 7):
            planted[m] = 2.0 * rng.standard_normal((2 * (L + 1 - m), D))
            a += w.wave_basis(lat, lon, m, L) @ planted[m]
        x = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
        M = len(lat_out)
        for mi, m in enumerate((1, 7)):
            parts = torch.empty((2, M, D), dtype=torch.float64, device=DEV)
            coef = torch.empty((2 * (L + 1 - m), D), dtype=torch.float64, device=DEV)
            one, dts = (C.c_void_p * 1)(x.data_ptr()), (C.c_int * 1)(0)
            _lib.check(lib.temxk_wave_project(h, mi, 1, one, dts, D, C.c_void_p(parts.data_ptr()), C.c_void_p(coef.data_ptr()), None))
            flag = C.c_int(7)
            _lib.check(lib.temxk_wave_status(h, C.byref(flag), None))
            e = fieldnorm_err(host(coef), planted[m])
            n = L + 1 - m
            Pz = w.pbar(m, L, np.sin(np.deg2rad(lat_out)))
            ep = fieldnorm_err(host(parts), np.stack([Pz @ planted[m][:n], Pz @ planted[m][n:]]))
            print("12x16 L=8 planted m=%d: coef %.2e parts %.2e" % (m, e, ep))
            assert flag.value == 0 and e <= TOL64 and ep <= TOL64, (m, flag.value, e, ep)
    finally:
        lib.temxk_wave_destroy(h)
    res_c, _ = plan.tem_run(*f)
    assert not plan.status()
    torch.cuda.synchronize()
    assert torch.equal(res_a, res_c)
    plan.close()
    # through Python: the library's error, with the wavenumber in the text
    with pytest.raises(_lib.TemxError, match="m = 8") as ei:
        TEMDiagnostics(*fnp, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=(8,))
    assert ei.value.code == -4
    Z = sph_zonal_averager(lat, lat_out, L, lon=lon, debug=False)
    Z.sph_compute_matrices()
    A = np.ascontiguousarray(fnp[0])
    with pytest.raises(_lib.TemxError, match="m = 8") as ei:
        Z.sph_wave(A, 8)
    assert ei.value.code == -4
    gc, gs = Z.sph_wave(A, 7)                                        # the averager is still good for the neighbour
    _, xc, xs = eddy_fit(lat, lon, lat_out, L, 7, A)
    e = fieldnorm_err(np.stack([gc, gs]), np.stack([xc, xs]))
    print("12x16 L=8 sph_wave m=7 after the refusal: %.2e" % e)
    assert e <= TOL64, e
    # 32 x 48 at L = 24
    lat, lon = synth.latlon_grid(32, 48)
    plan = engine.Plan(lat, lat_out, 24, device=0)
    rc, h = _create(lib, plan, lon, (24,))
    msg = err()
    assert rc == -4 and not h.value and b"m = 24" in msg and b"(pivot 1)" in msg, (rc, msg)
    rc, h = _create(lib, plan, lon, (23,))
    assert rc == 0 and h.value, err()
    lib.temxk_wave_destroy(h)
    plan.close()


# ---- 8: a non-finite value stays in its column and is reported ----------------------------------------------------------------------
def test_a_non_finite_value_stays_in_its_column_and_is_reported():
    """ne4 x 9 x 5 (D = 45), L = 12, wavenumbers (1, 2), one ``WaveState``.  A clean call, then NaN in ``wap`` at the last
    column of the grid (row N - 1, in the ragged last chunk) and d = 44 (the last live column of the last d-tile), then
    +inf in ``ua`` at row 0 and d = 17, then a clean call again.  Each poisoned call raises the flag once; every other
    column of flux and parts is bitwise that of the clean call; at column d the parts of the three untouched fields and the
    fluxes that do not involve the poisoned field are bitwise clean, the fluxes that do are non-finite."""
    from pytemdiags_amd import engine, synth, waves
    nlev, nt, L, ms = 9, 5, 12, (1, 2)
    D = nlev * nt
    lat, lon = synth.cubed_sphere_gll(4)
    N = lat.size
    plev = synth.pressure_levels(nlev)
    f = _dev(w.wave_fields(lat, lon, plev, nt))
    lat_out = orc.zm_latitudes(1)
    M = len(lat_out)
    plan = engine.Plan(lat, lat_out, L, device=0)
    plan.set_tem(nlev, nt, plev * 100)
    st = waves.WaveState(plan, lon, ms)
    try:
        flux0, parts0 = st.fluxes(*f, want_parts=True)
        assert not st.status()
        assert bool(torch.isfinite(flux0).all()) and bool(torch.isfinite(parts0).all())
        # (field poisoned, row, d, value, fluxes that do not involve it); fluxes: 0 u'v', 1 u'omega', 2 v'theta'
        for fi, row, d, val, clean_flux in ((3, N - 1, 44, float("nan"), (0, 2)), (0, 0, 17, float("inf"), (2,))):
            g = list(f)
            g[fi] = f[fi].clone()
            g[fi].view(N, D)[row, d] = val
            flux, parts = st.fluxes(*g, want_parts=True)
            assert st.status() and not st.status()
            fl, fl0 = flux.view(len(ms), 3, M, D), flux0.view(len(ms), 3, M, D)
            pt, pt0 = parts.view(len(ms), 4, 2, M, D), parts0.view(len(ms), 4, 2, M, D)
            others = [c for c in range(D) if c != d]
            assert torch.equal(fl[..., others], fl0[..., others]), (fi, "flux elsewhere")
            assert torch.equal(pt[..., others], pt0[..., others]), (fi, "parts elsewhere")
            for j in range(4):
                if j != fi:
                    assert torch.equal(pt[:, j, :, :, d], pt0[:, j, :, :, d]), (fi, "parts of field", j)
            assert not bool(torch.isfinite(pt[:, fi, :, :, d]).any()), (fi, "its own parts")
            for j in range(3):
                if j in clean_flux:
                    assert torch.equal(fl[:, j, :, d], fl0[:, j, :, d]), (fi, "flux", j)
                else:
                    assert not bool(torch.isfinite(fl[:, j, :, d]).any()), (fi, "flux", j)
            print("non-finite %r in %s at row %d, d = %d: confined to its column, flagged once" % (val, FIELDS[fi], row, d))
        flux1, parts1 = st.fluxes(*f, want_parts=True)
        assert not st.status()
        assert torch.equal(flux1, flux0) and torch.equal(parts1, parts0)
    finally:
        st.close()
        plan.close()


# ---- 9: one state, many calls, a side stream --------------------------------------------------------------------------------------------
def test_one_state_many_calls_on_a_side_stream():
    """ne4, L = 12, wavenumbers (1, 2, 4): one ``WaveState`` made and used under a stream other than the default --
    ``project`` at D = 15, ``project`` at D = 259 (the workspace grows), ``fluxes`` at D = 15, ``project`` at D = 15 again
    and ``fluxes`` again (the workspace is reused, larger than needed).  Each result is bitwise that of a fresh state that
    makes only that call on the default stream; ``workspace_bytes`` never shrinks and the repeated calls leave it alone."""
    from pytemdiags_amd import engine, synth, waves
    L, m = 12, 2
    lat, lon = synth.cubed_sphere_gll(4)
    lat_out = orc.zm_latitudes(1)
    plev = synth.pressure_levels(5)
    small = _dev(w.wave_fields(lat, lon, plev, 3))                               # D = 15
    large = torch.as_tensor(w.wave_fields(lat, lon, synth.pressure_levels(7), 37)[0], device=DEV)    # D = 259
    plan = engine.Plan(lat, lat_out, L, device=0)
    plan.set_tem(5, 3, plev * 100)

    def fresh(call):
        st = waves.WaveState(plan, lon, MS)
        try:
            out = call(st)
            assert not st.status()
            return out
        finally:
            st.close()

    calls = {"project15": lambda st: st.project(small[0], m, want_coef=True),
             "project259": lambda st: st.project(large, m, want_coef=True),
             "fluxes15": lambda st: st.fluxes(*small, want_parts=True)}
    try:
        want = {k: fresh(c) for k, c in calls.items()}
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
        got, nbytes = [], []
        with torch.cuda.stream(side):
            assert plan._stream().value == side.cuda_stream
            st = waves.WaveState(plan, lon, MS)
            try:
                nbytes.append(st.workspace_bytes)
                for k in ("project15", "project259", "fluxes15", "project15", "fluxes15"):
                    got.append((k, calls[k](st)))
                    nbytes.append(st.workspace_bytes)
                assert not st.status()                                   # (synchronises the side stream)
            finally:
                st.close()
        side.synchronize()
        for k, out in got:
            for a, b in zip(out, want[k]):
                assert torch.equal(a, b), k
        print("side stream: workspace bytes after create and the five calls: %s" % nbytes)
        assert all(b >= a for a, b in zip(nbytes, nbytes[1:])), nbytes
        assert nbytes[2] > nbytes[0] and nbytes[4] == nbytes[3] and nbytes[5] == nbytes[3], nbytes
    finally:
        plan.close()


# ---- 10: longitude conventions ------------------------------------------------------------------------------------------------------------
def test_longitude_conventions():
    """ne4, L = 12, m in (1, 4), ``sph_wave`` of one 3-D field.  Longitudes mapped to [-180, 180) and longitudes + 720
    name the same points: the parts agree with the original's.  Longitudes + 37 degrees rotate the frame: the amplitude
    ``hypot(Xc, Xs)`` is unchanged and the phase ``atan2(Xs, Xc) / m`` moves by ``deg2rad(37)`` modulo 2 pi / m
    (wrap-around distance, as in the planted test), where the amplitude is above 1e-3 of its maximum so that the phase is
    defined: that cut-off leaves out under 20 % of the points (asserted; near the poles a wave falls off as cos^m(lat))."""
    from pytemdiags_amd import sph_zonal_averager
    lat, lon, plev, f, L, ms, _ = w.case("ne4")
    lat_out = orc.zm_latitudes(1)
    A = np.array(f[1])                                               # (a copy: the cached fields are read-only)

    def parts(lon_deg):
        Z = sph_zonal_averager(lat, lat_out, L, lon=lon_deg, debug=False)
        Z.sph_compute_matrices()
        return {m: np.stack(Z.sph_wave(A, m)).astype(np.float64) for m in (1, 4)}

    base = parts(lon)
    signed = np.mod(lon + 180.0, 360.0) - 180.0
    assert signed.min() < 0.0 and lon.min() >= 0.0 and np.all(signed < 180.0)
    for name, other in (("[-180, 180)", parts(signed)), ("+ 720", parts(lon + 720.0))):
        for m in (1, 4):
            e = fieldnorm_err(other[m], base[m])
            print("lon %s m=%d parts: %.2e" % (name, m, e))
            assert e <= TOL64, (name, m, e)
    turned = parts(lon + 37.0)
    for m in (1, 4):
        amp0, amp1 = np.hypot(*base[m]), np.hypot(*turned[m])
        ea = fieldnorm_err(amp1, amp0)
        keep = amp0 > 1e-3 * amp0.max()
        left_out = 1.0 - keep.mean()
        ph0, ph1 = np.arctan2(base[m][1], base[m][0]) / m, np.arctan2(turned[m][1], turned[m][0]) / m
        dp = np.mod(ph1 - ph0 - np.deg2rad(37.0), 2 * np.pi / m)
        ep = float(np.max(np.minimum(dp, 2 * np.pi / m - dp)[keep]) / np.max(np.abs(ph0)))
        print("lon + 37 m=%d: amplitude %.2e phase %.2e (%.1f %% of the points left out)" % (m, ea, ep, 100 * left_out))
        assert left_out < 0.2, (m, left_out)
        assert ea <= TOL64 and ep <= TOL64, (m, ea, ep)
