"""The class form of the zonal-wavenumber fit on the MI355X: ``TEMDiagnostics(..., wave_form="classes")``,
``sph_zonal_averager(..., wave_form="classes").sph_wave``, ``waves.WaveState(..., form="classes")`` and the C ABI of
pytemdiags_amd/include_wavecls/temx_wavecls.h.

The reference is the numpy restatement of tests/test_gpu_wave.py, imported (``case``, ``reference``, ``check_front``,
``check_coefficients``, ``wave_fit``, ``wave_fields``): ``scipy.special.lpmv`` with the header's normalisation,
``np.linalg.lstsq`` on the explicit eddy of the oracle.  Where the oracle of a whole TEM run is not needed (the wide-D
cuts) the reference is ``wave_fit`` of ``x - ZonalAverager.zonal_mean_native(x)``, as in tests/test_gpu_wave_edges.py.
Bounds: the project's own, field-normalised (``conftest.fieldnorm_err``): ``TOL64 = 1e-10`` for fp64 and ``TOL32 = 2e-5``
for fp32 inputs (the fp32 reference is the restatement of the same fp32 values widened to fp64).  "Bitwise" is
``torch.equal``.  The cut a case means to exercise is asserted through ``temxz_wave_launch`` (``WaveState.launch``).

Instantiations (blocks of four degrees per parity of l - m): TBS = 2 on ne4 at L = 12 and on the lat-lon grid, 4 on ne8 at
L = 20 (m = 1, 3), 7 at L = 50 (m = 1, 3), 8 at L = 64 (m = 1, 64 degrees); each through the four-field sweep (front end)
and the one-field sweep (operator), fp64 and fp32.

Measured worst errors (MI355X, 256 CUs; every case prints its own):
  ne4 L = 12                   fp64 2.1e-12 (residual.dpsicoslat_dlat)   fp32 2.8e-07 (a set's epdiv)
  ne8 L = 20 (TBS 4)           fp64 2.8e-12 (m = 20, vptpb)              fp32 3.7e-07
  ne8 L = 50 (TBS 7)           fp64 8.3e-13                              fp32 1.8e-07
  ne8 L = 64 (TBS 8)           fp64 1.8e-12                              fp32 1.7e-07
  ne8 D = 259 / D = 2054       1.8e-13 (fp32 widened: 2.0e-13) / 2.3e-13; 30 and 15 pieces of the four-field sweep, 22 and
                               10 of their cuts inside a class-group
  lat-lon 24 x 48              18 pieces, 15 cuts inside a class-group
  a single piece               D = 26240 (1640 d-tiles); class form against generic form 9.7e-14 (coef), 1.2e-13 (parts)
  class form / generic form    ne4 1.7e-13 (fp32 1.3e-13), ne8 L = 50 2.6e-13 (2.8e-13), ne8 L = 65, m = 2 3.2e-14
  stored bytes, ne8 L = 50     generic state 7 466 372, class form 991 876
"""
import ctypes as C

import numpy as np
import pytest

import test_gpu_wave as w
from conftest import fieldnorm_err
from oracle import tem_oracle as orc
from test_gpu_wave import FIELDS, FLUXES, TOL32, TOL64, case, check_coefficients, check_front, host, reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = -7.25e300
PAD = 4096
_cache = {}


def _tol(dtype):
    return TOL64 if np.dtype(dtype) == np.float64 else TOL32


def _dev(fields):
    return [torch.tensor(x, device=DEV) for x in fields]            # (a copy: the cached fields are read-only)


def any_case(kind, dtype=np.float64, desc=False):
    """``case`` of tests/test_gpu_wave.py, plus ne8 x 4 x 2 at L = 64, m = 1 (64 degrees: the widest basis the class form
    serves; cond(Ym) lies between the 2.5 of L = 60 and the 3.5 of L = 70)."""
    if kind != "ne8L64":
        return case(kind, dtype, desc)
    from pytemdiags_amd import synth
    key = (kind, np.dtype(dtype).name)
    if key not in _cache:
        lat, lon = synth.cubed_sphere_gll(8)
        plev = synth.pressure_levels(4)
        f = w.wave_fields(lat, lon, plev, 2, dtype=dtype)
        for x in f:
            x.setflags(write=False)
        _cache[key] = (lat, lon, plev, f, 64, (1,))
    lat, lon, plev, f, L, ms = _cache[key]
    return lat, lon, plev, f, L, ms, reference(("wavecls",) + key, lat, lon, plev, f, L, ms)


def run_classes(kind, dtype=np.float64, desc=False):
    """The front end in the class form, once per shape."""
    from pytemdiags_amd import TEMDiagnostics
    key = ("tem", kind, np.dtype(dtype).name, desc)
    lat, lon, plev, f, L, ms, ref = any_case(kind, dtype, desc)
    if key not in _cache:
        _cache[key] = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms, wave_form="classes")
    tem = _cache[key]
    assert tem.waves.form == "classes" and tem.waves.wavenumbers == tuple(ms)
    return tem, ref


def class_coefficients(monkeypatch, tem, ref, lon, ms, tol, tag):
    """``check_coefficients`` of tests/test_gpu_wave.py with its state in the class form."""
    from pytemdiags_amd import waves
    generic = waves.WaveState
    monkeypatch.setattr(waves, "WaveState", lambda plan, lo, m: generic(plan, lo, m, form="classes"))
    check_coefficients(tem, ref, lon, ms, tol, tag)


def eddy_fit(lat, lon, lat_out, L, m, x64, Zo):
    return w.wave_fit(x64 - Zo.zonal_mean_native(x64), lat, lon, lat_out, m, L)


def fluxes_of(parts):
    xc, xs = parts[:, 0], parts[:, 1]
    return np.stack([0.5 * (xc[0] * xc[1] + xs[0] * xs[1]), 0.5 * (xc[0] * xc[3] + xs[0] * xs[3]),
                     0.5 * (xc[1] * xc[2] + xs[1] * xs[2])])


# ---- parity on the small shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_parity_smallest_shape_coefficients_parts_fluxes_sets_residual(dtype, monkeypatch):
    """ne4 (866 columns) x 5 x 3 (D = 15), L = 12, wavenumbers (1, 2, 4): sides of 1 (the poles), 4 and 8 members and an
    equator class with one side only.  Wave 4 is there for the deflation term: a fit of the raw field is off by a factor
    of 11 there."""
    from pytemdiags_amd import _wavecls
    tem, ref = run_classes("ne4", dtype)
    lat, lon, plev, f, L, ms, _ = any_case("ne4", dtype)
    assert all(_wavecls.shape(L, m)["TBS"] == 2 for m in ms) and tem.waves.workspace_bytes > 0
    tag = "classes ne4 %s" % np.dtype(dtype).name
    check_front(tem, ref, ms, _tol(dtype), tag)
    class_coefficients(monkeypatch, tem, ref, lon, ms, _tol(dtype), tag)


@pytest.mark.parametrize("desc", [False, True], ids=["ascending", "descending-plev"])
def test_parity_three_d_tiles_with_a_tail_and_a_basis_of_one_degree(desc):
    """ne8 x 9 x 5 (D = 45: three d-tiles, the last with 13 columns), L = 20, wavenumbers (1, 3, 20): at m = L there is one
    degree, every odd-parity block is empty."""
    from pytemdiags_amd import _wavecls
    tem, ref = run_classes("ne8", desc=desc)
    assert _wavecls.shape(20, 20) == dict(ndeg=1, Kc=2, TBS=2, nacc=8, fpw=1)
    check_front(tem, ref, tem.waves.wavenumbers, TOL64, "classes ne8 desc=%s" % desc)


# ---- every instantiation, both entry points, both dtypes ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind,tbs", [("ne8", 4), ("ne8L50", 7), ("ne8L64", 8)], ids=["TBS4", "TBS7", "TBS8-64-degrees"])
def test_every_instantiation_through_both_entry_points(kind, tbs, dtype, monkeypatch):
    """TBS = 4 (ne8 x 9 x 5, L = 20), 7 (ne8 x 4 x 2, L = 50, m = 1 and 3) and 8 (L = 64, m = 1: 64 degrees, the widest
    basis served); TBS = 2 is the ne4 test.  The front end runs the four-field sweep, the coefficients the one-field one."""
    from pytemdiags_amd import _wavecls, waves
    lat, lon, plev, f, L, ms, ref = any_case(kind, dtype)
    assert _wavecls.shape(L, ms[0])["TBS"] == tbs
    tem, _ = run_classes(kind, dtype)
    st = waves.WaveState(tem.ZM._plan, lon, ms, form="classes")
    try:
        D = tem.ua.shape[1] * tem.ua.shape[2]
        assert st.launch(ms[0], 4, D)["TBS"] == tbs and st.launch(ms[0], 1, D)["TBS"] == tbs
    finally:
        st.close()
    tag = "classes %s %s" % (kind, np.dtype(dtype).name)
    check_front(tem, ref, ms, _tol(dtype), tag)
    class_coefficients(monkeypatch, tem, ref, lon, ms, _tol(dtype), tag)


def test_65_degrees_are_refused_and_the_plan_stays_usable():
    """ne8 at L = 65: m = 1 has 65 degrees and is refused by the C ABI (TEMX_EUNSUPPORTED, no state) and by the front end
    (ValueError naming the generic form); m = 2 (64 degrees) is served on the same plan afterwards, as is the generic
    form at m = 1, and the two agree at m = 2."""
    from pytemdiags_amd import TEMDiagnostics, _wavecls, engine, synth, waves
    lib = _wavecls.load()
    lat, lon = synth.cubed_sphere_gll(8)
    lat_out = orc.zm_latitudes(1)
    plan = engine.Plan(lat, lat_out, 65, device=0)
    try:
        h = C.c_void_p()
        rc = lib.temxz_wave_create(C.byref(h), plan._h, np.ascontiguousarray(lon).ctypes.data_as(C.POINTER(C.c_double)), 1,
                                   (C.c_int * 1)(1))
        assert rc == -6 and not h.value and b"65 degrees" in lib.temx_last_error() and b"generic form" in lib.temx_last_error()
        with pytest.raises(ValueError, match="generic form"):
            waves.WaveState(plan, lon, (1,), form="classes")
        x = torch.tensor(w.wave_fields(lat, lon, synth.pressure_levels(4), 2)[0], device=DEV)
        gen = waves.WaveState(plan, lon, (1, 2))
        cls = waves.WaveState(plan, lon, (2,), form="classes")
        try:
            assert bool(torch.isfinite(gen.project(x, 1)).all())
            pg, cg = gen.project(x, 2, want_coef=True)
            pc, cc = cls.project(x, 2, want_coef=True)
            assert cls.launch(2, 1, 8)["TBS"] == 8 and not cls.status() and not gen.status()
            e = max(fieldnorm_err(host(pc), host(pg)), fieldnorm_err(host(cc), host(cg)))
            print("L = 65, m = 2 (64 degrees), class form against generic form: %.2e" % e)
            assert e <= TOL64
        finally:
            gen.close()
            cls.close()
    finally:
        plan.close()
    plev = synth.pressure_levels(4)
    f = w.wave_fields(lat, lon, plev, 2)
    with pytest.raises(ValueError, match="generic form"):
        TEMDiagnostics(*f, lat, plev=plev, L=65, debug_level=0, lon=lon, wavenumbers=(1,), wave_form="classes")


# ---- lat-lon: planted coefficients, long sides, a cut inside a class-group -------------------------------------------------------
def _planted(dtype):
    from pytemdiags_amd import synth
    key = ("planted", np.dtype(dtype).name)
    if key not in _cache:
        L, ms, nlev, nt = 10, (1, 4, 10), 3, 2
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
                a += w.wave_basis(lat, lon, m, L) @ c
            fields.append(np.ascontiguousarray(a.reshape(len(lat), nlev, nt).astype(dtype)))
        _cache[key] = (lat, lon, plev, fields, planted, L, ms, nlev, nt)
    return _cache[key]


def test_planted_coefficients_come_back_with_amplitude_and_phase_on_long_sides():
    """lat-lon 24 x 48, L = 10, wavenumbers (1, 4, 10), fp64: 12 classes of 48 + 48 members, twelve batches per side, three
    class-groups of 24 batches -- so every cut but two falls inside a class-group, which ``temxz_wave_launch`` confirms
    for both sweeps.  Fields built from random coefficients plus zonally symmetric parts; cos(m lon) is exactly
    orthogonal to the zonal harmonics here."""
    from pytemdiags_amd import TEMDiagnostics, waves
    lat, lon, plev, fields, planted, L, ms, nlev, nt = _planted(np.float64)
    tem = TEMDiagnostics(*fields, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms, wave_form="classes")
    st = waves.WaveState(tem.ZM._plan, lon, ms, form="classes")
    try:
        for nf in (4, 1):
            la = st.launch(ms[0], nf, nlev * nt)
            print("lat-lon 24 x 48, nf = %d: %s" % (nf, la))
            assert la["TBS"] == 2 and la["ndt"] == 1 and la["pieces"] > 3 and la["inside"] >= la["pieces"] - 3
        for f, x in enumerate((tem.ua, tem.va, tem.ta, tem.wap)):
            for m in ms:
                _, coef = st.project(x, m, want_coef=True)
                e = fieldnorm_err(host(coef), planted[(f, m)])
                print("classes planted f=%d m=%d coef: %.2e" % (f, m, e))
                assert e <= TOL64, (f, m, e)
        assert not st.status()
    finally:
        st.close()
    lat_out = tem.lat
    for m in ms:
        Pz = w.pbar(m, L, np.sin(np.deg2rad(lat_out)))
        n = L + 1 - m
        for f, name in ((0, "ua"), (1, "va"), (3, "wap")):     # (theta carries the factor (p0/p)^kappa per level)
            xc = (Pz @ planted[(f, m)][:n]).reshape(len(lat_out), nlev, nt)
            xs = (Pz @ planted[(f, m)][n:]).reshape(len(lat_out), nlev, nt)
            ea = fieldnorm_err(host(tem.waves[m].amplitude(name)), np.hypot(xc, xs))
            ph = np.arctan2(xs, xc) / m
            dp = np.abs(host(tem.waves[m].phase(name)) - ph)
            ep = float(np.max(np.minimum(dp, 2 * np.pi / m - dp)) / np.max(np.abs(ph)))
            print("classes planted m=%d %s amplitude %.2e phase %.2e" % (m, name, ea, ep))
            assert ea <= TOL64 and ep <= TOL64, (m, name, ea, ep)
    th = (tem.p0 / (plev * 100)) ** orc.k
    for m in ms:
        Pz = w.pbar(m, L, np.sin(np.deg2rad(lat_out)))
        n = L + 1 - m
        c = planted[(2, m)].reshape(-1, nlev, nt) * th[None, :, None]
        xc, xs = np.tensordot(Pz, c[:n], 1), np.tensordot(Pz, c[n:], 1)
        assert fieldnorm_err(host(tem.waves[m].amplitude("theta")), np.hypot(xc, xs)) <= TOL64


def test_fp32_plan_with_sides_cut_into_parts_of_eight():
    """The same grid and fields in fp32: the plan made for fp32 fields cuts the sides of 48 into parts of 8, six classes
    at every latitude (72 classes in 18 groups; tests/test_wavecls_host.py checks that table), each with the basis and
    the deflation rows of its latitude.  Against the restatement on the fp32 values widened to fp64."""
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, fields, _, L, ms, nlev, nt = _planted(np.float32)
    tem = TEMDiagnostics(*fields, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms, wave_form="classes")
    assert tem.ua.dtype == torch.float32 and tem.waves.form == "classes"
    Zo = orc.ZonalAverager(lat, tem.lat, L, mode="factorised")
    th = ((tem.p0 / (plev * 100)) ** orc.k)[None, :, None]
    x64 = np.stack([np.asarray(x, dtype=np.float64) * (th if i == 2 else 1.0) for i, x in enumerate(fields)], axis=1)
    worst = 0.0
    for m in ms:
        _, xc, xs = eddy_fit(lat, lon, tem.lat, L, m, x64, Zo)
        want = np.stack([xc, xs]).transpose(2, 0, 1, 3, 4)                      # [4][2][M][nlev][nt]
        for i, name in enumerate(FIELDS):
            gc, gs = tem.waves[m].parts(name)
            e = fieldnorm_err(np.stack([host(gc), host(gs)]), want[i])
            print("classes lat-lon fp32 m=%d parts(%s): %.2e" % (m, name, e))
            worst = max(worst, e)
        for j, r in enumerate(fluxes_of(want)):
            e = fieldnorm_err(host(getattr(tem.waves[m], FLUXES[j])), r)
            print("classes lat-lon fp32 m=%d flux %s: %.2e" % (m, FLUXES[j], e))
            worst = max(worst, e)
    assert worst <= TOL32, worst


# ---- cuts ----------------------------------------------------------------------------------------------------------------------
def test_a_single_piece():
    """The one-field sweep over so many columns that the row table is not cut at all (the d-tiles alone fill the device):
    the smallest multiple of 64 columns for which ``temxz_wave_launch`` reports one piece, an fp32 field of ne4 made on the
    device.  The reference is the generic form on the same field (itself held to the restatement elsewhere); the bound is
    that of fp32 inputs."""
    from pytemdiags_amd import engine, synth, waves
    L, m = 12, 2
    lat, lon = synth.cubed_sphere_gll(4)
    plan = engine.Plan(lat, orc.zm_latitudes(1), L, device=0, fp32_fields=True)
    cls = waves.WaveState(plan, lon, (m,), form="classes")
    gen = waves.WaveState(plan, lon, (m,))
    try:
        D = next((64 * j for j in range(1, 4097) if cls.launch(m, 1, 64 * j)["pieces"] == 1), None)
        assert D is not None, "no D up to 2^18 runs the one-field sweep in one piece"
        la = cls.launch(m, 1, D)
        print("single piece: D = %d, %s" % (D, la))
        assert la["pieces"] == 1 and la["inside"] == 0 and la["ndt"] == D // 16
        g = torch.Generator(device=DEV).manual_seed(5)
        lam = torch.tensor(np.deg2rad(lon), device=DEV)[:, None]
        x = (250.0 + 3.0 * torch.cos(m * lam + torch.arange(D, device=DEV)[None, :] * 0.01)
             + 0.1 * torch.randn((lat.size, D), generator=g, device=DEV, dtype=torch.float64)).to(torch.float32)
        pc, cc = cls.project(x, m, want_coef=True)
        pg, cg = gen.project(x, m, want_coef=True)
        assert not cls.status() and not gen.status()
        e, ep = fieldnorm_err(host(cc), host(cg)), fieldnorm_err(host(pc), host(pg))
        print("single piece: class form against generic form, coef %.2e parts %.2e" % (e, ep))
        assert e <= TOL32 and ep <= TOL32 and float(cc.abs().max()) > 1.0
    finally:
        cls.close()
        gen.close()
        plan.close()
        torch.cuda.empty_cache()


class TestWideD:
    """ne8 (3458 columns, 219 batches in 62 class-groups), L = 20, m = 1 and 3 (TBS = 4), against ``wave_fit`` of the
    explicit eddy: ``WaveState.fluxes`` with parts after ``plan.set_tem`` and ``WaveState.project`` of ``ua`` with
    coefficients.  D = 259 (7 x 37: 17 d-tiles, the last with 3 columns, a ragged workgroup of the one-field sweep and
    launch blocks of the solve and the parts beyond the first) and D = 2054 (13 x 158: 129 d-tiles, few pieces of many
    batches each)."""

    @pytest.mark.parametrize("nlev,nt,dtype", [(7, 37, np.float64), (7, 37, np.float32), (13, 158, np.float64)],
                             ids=["D259-fp64", "D259-fp32", "D2054-fp64"])
    def test_launch_blocks_beyond_the_first_and_many_batches_per_piece(self, nlev, nt, dtype):
        from pytemdiags_amd import engine, synth, waves
        L, ms = 20, (1, 3)
        lat, lon = synth.cubed_sphere_gll(8)
        plev = synth.pressure_levels(nlev)
        D = nlev * nt
        f = w.wave_fields(lat, lon, plev, nt, dtype=dtype)
        lat_out = orc.zm_latitudes(1)
        tol, tag = _tol(dtype), "classes ne8 D=%d %s" % (D, np.dtype(dtype).name)
        plan = engine.Plan(lat, lat_out, L, device=0)
        plan.set_tem(nlev, nt, plev * 100, p0=orc.P0)
        dev = _dev(f)
        st = waves.WaveState(plan, lon, ms, form="classes")
        try:
            l4, l1 = st.launch(1, 4, D), st.launch(1, 1, D)
            print("%s: four-field sweep %s, one-field sweep %s" % (tag, l4, l1))
            assert l4["ndt"] == l1["ndt"] == (D + 15) // 16 and l4["TBS"] == 4 and D % 16 in (3, 6)
            assert 219 // l4["pieces"] >= (2 if D == 259 else 8), l4        # batches per piece
            flux, parts = st.fluxes(*dev, want_parts=True)
            got = {m: st.project(dev[0], m, want_coef=True) for m in ms}
            assert not st.status()
            flux, parts = host(flux), host(parts)
            got = {m: (host(p), host(c)) for m, (p, c) in got.items()}
        finally:
            st.close()
            plan.close()
            del dev
            torch.cuda.empty_cache()
        Zo = orc.ZonalAverager(lat, lat_out, L, mode="factorised")
        th = ((orc.P0 / (plev * 100)) ** orc.k)[None, :, None]
        x64 = np.stack([np.asarray(x, dtype=np.float64) * (th if i == 2 else 1.0) for i, x in enumerate(f)], axis=1)
        worst = (0.0, "")
        for mi, m in enumerate(ms):
            c, xc, xs = eddy_fit(lat, lon, lat_out, L, m, x64, Zo)
            c = c.reshape(c.shape[0], 4, D)
            want = np.stack([xc, xs]).transpose(2, 0, 1, 3, 4)
            for i in range(4):
                worst = max(worst, (fieldnorm_err(parts[mi, i], want[i]), "m%d.parts.%s" % (m, FIELDS[i])))
            for j, r in enumerate(fluxes_of(want)):
                worst = max(worst, (fieldnorm_err(flux[mi, j], r), "m%d.%s" % (m, FLUXES[j])))
            worst = max(worst, (fieldnorm_err(got[m][1], c[:, 0]), "m%d.coef.ua" % m),
                        (fieldnorm_err(got[m][0], want[0]), "m%d.project.parts.ua" % m))
        print("%s: worst field-normalised error %.2e (%s)" % (tag, worst[0], worst[1]))
        assert worst[0] <= tol, (tag, worst)


# ---- the two forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("kind", ["ne4", "ne8L50"])
def test_agreement_with_the_generic_form_on_the_same_inputs(kind, dtype):
    """Fluxes, parts and coefficients of the two forms, states on one plan and the same device fields."""
    from pytemdiags_amd import waves
    tem, _ = run_classes(kind, dtype)
    lat, lon, plev, f, L, ms, _ = any_case(kind, dtype)
    plan, dev = tem.ZM._plan, (tem.ua, tem.va, tem.ta, tem.wap)
    cls, gen = waves.WaveState(plan, lon, ms, form="classes"), waves.WaveState(plan, lon, ms)
    try:
        fc, pc = cls.fluxes(*dev, want_parts=True)
        fg, pg = gen.fluxes(*dev, want_parts=True)
        worst = 0.0
        for i in range(len(ms)):
            worst = max([worst] + [fieldnorm_err(host(fc[i, j]), host(fg[i, j])) for j in range(3)]
                        + [fieldnorm_err(host(pc[i, j]), host(pg[i, j])) for j in range(4)])
            _, cc = cls.project(tem.ua, ms[i], want_coef=True)
            _, cg = gen.project(tem.ua, ms[i], want_coef=True)
            worst = max(worst, fieldnorm_err(host(cc), host(cg)))
        assert not cls.status() and not gen.status()
        print("%s %s: class form against generic form %.2e" % (kind, np.dtype(dtype).name, worst))
        assert worst <= _tol(dtype), worst
    finally:
        cls.close()
        gen.close()


@pytest.mark.parametrize("kind", ["ne4", "ne8"])
def test_sets_plus_residual_add_up_to_the_ordinary_run(kind):
    tem, _ = run_classes(kind)
    for n in w.ADDITIVE:
        total = host(getattr(tem, n)())
        s = host(getattr(tem.waves.residual, n)())
        for m in tem.waves.wavenumbers:
            s = s + host(getattr(tem.waves[m], n)())
        e = fieldnorm_err(s, total)
        print("classes %s closure %s: %.2e" % (kind, n, e))
        assert e <= 1e-10, (kind, n, e)


def test_the_ordinary_run_is_bit_identical_whatever_the_form_and_runs_repeat():
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f, L, ms, _ = case("ne4")
    a, _ = run_classes("ne4")
    b = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms, wave_form="classes")
    g = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, lon=lon, wavenumbers=ms, wave_form="generic")
    plain = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0)
    assert g.waves.form == "generic"
    va, vb, vg, vp = (w.set_values(t) for t in (a, b, g, plain))
    for n in va:
        assert np.array_equal(va[n], vp[n]) and np.array_equal(va[n], vg[n]) and np.array_equal(va[n], vb[n]), n
    for m in ms:                                      # two runs of the class form: bitwise
        wa, wb = w.set_values(a.waves[m]), w.set_values(b.waves[m])
        assert all(np.array_equal(wa[n], wb[n]) for n in wa), m
        for name in FIELDS:
            for x, y in zip(a.waves[m].parts(name), b.waves[m].parts(name)):
                assert np.array_equal(host(x), host(y)), (m, name)
    ra, rb = w.set_values(a.waves.residual), w.set_values(b.waves.residual)
    assert all(np.array_equal(ra[n], rb[n]) for n in ra)


def test_one_state_many_calls_on_a_side_stream():
    """One class-form state made and used under a side stream: ``project`` at D = 15, at D = 259 (the workspace grows),
    ``fluxes`` at D = 15 and both again.  Each result is bitwise that of a fresh state that makes only that call on the
    default stream; ``workspace_bytes`` never shrinks."""
    from pytemdiags_amd import engine, synth, waves
    L, m, MS = 12, 2, (1, 2, 4)
    lat, lon = synth.cubed_sphere_gll(4)
    plev = synth.pressure_levels(5)
    small = _dev(w.wave_fields(lat, lon, plev, 3))
    large = torch.as_tensor(w.wave_fields(lat, lon, synth.pressure_levels(7), 37)[0], device=DEV)
    plan = engine.Plan(lat, orc.zm_latitudes(1), L, device=0)
    plan.set_tem(5, 3, plev * 100)

    def fresh(call):
        st = waves.WaveState(plan, lon, MS, form="classes")
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
        got, nbytes = [], []
        with torch.cuda.stream(side):
            assert plan._stream().value == side.cuda_stream
            st = waves.WaveState(plan, lon, MS, form="classes")
            try:
                nbytes.append(st.workspace_bytes)
                for k in ("project15", "project259", "fluxes15", "project15", "fluxes15"):
                    got.append((k, calls[k](st)))
                    nbytes.append(st.workspace_bytes)
                assert not st.status()
            finally:
                st.close()
        side.synchronize()
        for k, out in got:
            for x, y in zip(out, want[k]):
                assert torch.equal(x, y), k
        assert all(y >= x for x, y in zip(nbytes, nbytes[1:])) and nbytes[2] > nbytes[0] and nbytes[5] == nbytes[3], nbytes
    finally:
        plan.close()


# ---- guards, a NaN --------------------------------------------------------------------------------------------------------------
def _guarded(n):
    big = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float64, device=DEV)
    return big, big[PAD:PAD + n]


def _guards_untouched(big, n):
    want = torch.full((PAD,), CANARY, dtype=torch.float64, device=DEV)
    return torch.equal(big[:PAD], want) and torch.equal(big[PAD + n:], want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_guard_values_around_every_output_are_intact(dtype):
    """ne4 x 7 x 37 (D = 259) through the C ABI, every output inside a tensor of canaries with 4096 doubles in front and
    behind: the guards stay bitwise, every entry inside is overwritten and is bitwise that of the exact-size call."""
    from pytemdiags_amd import _lib, engine, synth, waves
    nlev, nt, L, MS = 7, 37, 12, (1, 2, 4)
    D = nlev * nt
    lat, lon = synth.cubed_sphere_gll(4)
    plev = synth.pressure_levels(nlev)
    lat_out = orc.zm_latitudes(1)
    M = len(lat_out)
    plan = engine.Plan(lat, lat_out, L, device=0)
    plan.set_tem(nlev, nt, plev * 100, p0=orc.P0)
    dev = _dev(w.wave_fields(lat, lon, plev, nt, dtype=dtype))
    dt = engine._DT[dev[0].dtype]
    st = waves.WaveState(plan, lon, MS, form="classes")
    lib = st.lib
    ptr = lambda t: C.c_void_p(t.data_ptr())
    try:
        flux_ref, parts_ref = st.fluxes(*dev, want_parts=True)
        nfl, npt = len(MS) * 3 * M * D, len(MS) * 8 * M * D
        bf, flux = _guarded(nfl)
        bp, parts = _guarded(npt)
        _lib.check(lib.temxz_wave_fluxes(st._h, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), dt, ptr(flux), ptr(parts), None))
        torch.cuda.synchronize()
        assert _guards_untouched(bf, nfl) and _guards_untouched(bp, npt)
        assert torch.equal(flux, flux_ref.reshape(-1)) and torch.equal(parts, parts_ref.reshape(-1))
        for mi, m in enumerate(MS):
            Kc = 2 * (L + 1 - m)
            p_ref, c_ref = st.project(dev[3], m, want_coef=True)
            bq, pj = _guarded(2 * M * D)
            bc, coef = _guarded(Kc * D)
            one, dts = (C.c_void_p * 1)(dev[3].data_ptr()), (C.c_int * 1)(dt)
            _lib.check(lib.temxz_wave_project(st._h, mi, 1, one, dts, D, ptr(pj), ptr(coef), None))
            torch.cuda.synchronize()
            assert _guards_untouched(bq, 2 * M * D) and _guards_untouched(bc, Kc * D), m
            assert torch.equal(pj, p_ref.reshape(-1)) and torch.equal(coef, c_ref.reshape(-1)), m
        assert not st.status()
    finally:
        st.close()
        plan.close()


def test_a_nan_stays_in_its_column_and_is_reported():
    """ne4 x 9 x 5 (D = 45), L = 12, wavenumbers (1, 2).  NaN in ``wap`` at the last column of the grid and d = 44, then
    +inf in ``ua`` at row 0 (the row padding entries read) and d = 17: each call raises the state's flag once, every
    other column is bitwise that of the clean call, and at column d only what involves the poisoned field is non-finite.
    The plan's own flag stays down."""
    from pytemdiags_amd import engine, synth, waves
    nlev, nt, L, ms = 9, 5, 12, (1, 2)
    D = nlev * nt
    lat, lon = synth.cubed_sphere_gll(4)
    N = lat.size
    plev = synth.pressure_levels(nlev)
    f = _dev(w.wave_fields(lat, lon, plev, nt))
    M = len(orc.zm_latitudes(1))
    plan = engine.Plan(lat, orc.zm_latitudes(1), L, device=0)
    plan.set_tem(nlev, nt, plev * 100)
    st = waves.WaveState(plan, lon, ms, form="classes")
    try:
        flux0, parts0 = st.fluxes(*f, want_parts=True)
        assert not st.status() and bool(torch.isfinite(flux0).all()) and bool(torch.isfinite(parts0).all())
        for fi, row, d, val, clean_flux in ((3, N - 1, 44, float("nan"), (0, 2)), (0, 0, 17, float("inf"), (2,))):
            g = list(f)
            g[fi] = f[fi].clone()
            g[fi].view(N, D)[row, d] = val
            flux, parts = st.fluxes(*g, want_parts=True)
            assert st.status() and not st.status() and not plan.status()
            fl, fl0 = flux.view(len(ms), 3, M, D), flux0.view(len(ms), 3, M, D)
            pt, pt0 = parts.view(len(ms), 4, 2, M, D), parts0.view(len(ms), 4, 2, M, D)
            others = [c for c in range(D) if c != d]
            assert torch.equal(fl[..., others], fl0[..., others]) and torch.equal(pt[..., others], pt0[..., others]), fi
            for j in range(4):
                if j != fi:
                    assert torch.equal(pt[:, j, :, :, d], pt0[:, j, :, :, d]), (fi, "parts of field", j)
            assert not bool(torch.isfinite(pt[:, fi, :, :, d]).any()), (fi, "its own parts")
            for j in range(3):
                if j in clean_flux:
                    assert torch.equal(fl[:, j, :, d], fl0[:, j, :, d]), (fi, "flux", j)
                else:
                    assert not bool(torch.isfinite(fl[:, j, :, d]).any()), (fi, "flux", j)
        flux1, parts1 = st.fluxes(*f, want_parts=True)
        assert not st.status() and torch.equal(flux1, flux0) and torch.equal(parts1, parts0)
    finally:
        st.close()
        plan.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_a_grid_without_repeated_latitudes_is_refused_and_keeps_the_generic_form():
    """ne4 with every latitude moved by up to 1e-3 degrees: no two columns share a latitude, the plan holds no class tables.
    The C ABI refuses with TEMX_EUNSUPPORTED and makes no state, the front end raises a ValueError that names the
    generic form, and the same plan serves the generic form afterwards."""
    from pytemdiags_amd import TEMDiagnostics, _wavecls, engine, synth, waves
    lib = _wavecls.load()
    lat, lon = synth.cubed_sphere_gll(4)
    rng = np.random.default_rng(11)
    lat = np.clip(lat + 1e-3 * rng.uniform(-1, 1, lat.size), -90.0, 90.0)
    plev = synth.pressure_levels(3)
    f = w.wave_fields(lat, lon, plev, 2)
    plan = engine.Plan(lat, orc.zm_latitudes(1), 12, device=0)
    try:
        h = C.c_void_p()
        rc = lib.temxz_wave_create(C.byref(h), plan._h, np.ascontiguousarray(lon).ctypes.data_as(C.POINTER(C.c_double)), 1,
                                   (C.c_int * 1)(1))
        assert rc == -6 and not h.value and b"latitude classes" in lib.temx_last_error()
        with pytest.raises(ValueError, match="generic form"):
            waves.WaveState(plan, lon, (1,), form="classes")
        gen = waves.WaveState(plan, lon, (1,))
        try:
            assert bool(torch.isfinite(gen.project(torch.tensor(f[0], device=DEV), 1)).all()) and not gen.status()
        finally:
            gen.close()
    finally:
        plan.close()
    with pytest.raises(ValueError, match="generic form"):
        TEMDiagnostics(*f, lat, plev=plev, L=12, debug_level=0, lon=lon, wavenumbers=(1,), wave_form="classes")
    assert TEMDiagnostics(*f, lat, plev=plev, L=12, debug_level=0, lon=lon, wavenumbers=(1,)).waves.form == "generic"


def test_c_abi_refusals_as_in_the_generic_form_leave_the_plan_usable():
    from pytemdiags_amd import _wavecls, engine, synth
    lib = _wavecls.load()
    err = lib.temx_last_error
    lat, lon = synth.cubed_sphere_gll(4)
    lat_out = orc.zm_latitudes(1)
    lon_p = np.ascontiguousarray(lon).ctypes.data_as(C.POINTER(C.c_double))

    def create(plan, ms, lon_ptr=lon_p, nm=None):
        h = C.c_void_p()
        arr = (C.c_int * max(1, len(ms)))(*ms)
        rc = lib.temxz_wave_create(C.byref(h), plan._h if plan is not None else None, lon_ptr, len(ms) if nm is None else nm, arr)
        assert (rc == 0) == bool(h.value)
        return rc, h

    plan = engine.Plan(lat, lat_out, 12, device=0)
    assert create(None, (1,))[0] == -1 and create(plan, (1,), lon_ptr=None)[0] == -1
    assert create(plan, (), nm=0)[0] == -1 and b"nm" in err()
    assert create(plan, (0,))[0] == -1 and b"1..L" in err()
    assert create(plan, (13,))[0] == -1 and b"1..L" in err()
    assert create(plan, (2, 3, 2))[0] == -1 and b"twice" in err()
    bad = np.array(lon)
    bad[5] = np.nan
    assert create(plan, (1,), lon_ptr=bad.ctypes.data_as(C.POINTER(C.c_double)))[0] == -1 and b"lon 5" in err()
    deferred = engine.Plan(lat, lat_out, 12, device=0, defer_finalize=True)
    assert create(deferred, (1,))[0] == -5 and b"finalised" in err()
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
    rc, h = create(plan, (1, 4))
    assert rc == 0 and lib.temxz_wave_workspace_bytes(h) > 0
    nlev, nt = 3, 2
    plev = synth.pressure_levels(nlev)
    f = [torch.as_tensor(x, device=DEV) for x in w.wave_fields(lat, lon, plev, nt)]
    M, D = len(lat_out), nlev * nt
    flux = torch.empty((2, 3, M, nlev, nt), dtype=torch.float64, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    fl = lambda dt=0, out=flux, u=f[0]: lib.temxz_wave_fluxes(h, ptr(u) if u is not None else None, ptr(f[1]), ptr(f[2]), ptr(f[3]), dt,
                                                              ptr(out) if out is not None else None, None, None)
    assert fl() == -5 and b"temx_plan_set_tem" in err()
    plan.set_tem(nlev, nt, plev * 100)
    assert fl(dt=2) == -1 and b"dtype" in err() and fl(out=None) == -1 and fl(u=None) == -1
    parts = torch.empty((2, M, D), dtype=torch.float64, device=DEV)
    one, dts = (C.c_void_p * 1)(f[0].data_ptr()), (C.c_int * 1)(0)
    pj = lambda mi=0, nf=1, fields=one, dt=dts, Dv=D, out=parts: lib.temxz_wave_project(
        h, mi, nf, fields, dt, Dv, ptr(out) if out is not None else None, None, None)
    assert pj(mi=2) == -1 and b"mi" in err() and pj(mi=-1) == -1
    assert pj(nf=0) == -1 and pj(nf=9) == -1 and b"nf" in err()
    assert pj(fields=None) == -1 and pj(dt=None) == -1 and pj(out=None) == -1
    assert pj(fields=(C.c_void_p * 1)(None)) == -1
    assert pj(dt=(C.c_int * 1)(7)) == -1 and b"dtype" in err()
    assert pj(Dv=0) == -1 and b"D must" in err()
    out4 = (C.c_int * 4)()
    assert lib.temxz_wave_launch(h, 2, 4, D, out4) == -1 and lib.temxz_wave_launch(h, 0, 3, D, out4) == -1 and b"nf" in err()
    assert lib.temxz_wave_launch(h, 0, 4, 0, out4) == -1 and lib.temxz_wave_launch(h, 0, 4, D, None) == -1
    assert fl() == 0 and pj() == 0
    res_a, _ = plan.tem_run(*f)
    plan.configure(missing="mask")
    assert fl() == -5
    plan.set_tem(nlev, nt, plev * 100)
    assert fl() == -6 and b"missing" in err()
    plan.configure(missing="raise")
    plan.set_tem(nlev, nt, plev * 100)
    flux2 = torch.empty_like(flux)
    assert fl(out=flux2) == 0
    res_b, _ = plan.tem_run(*f)
    torch.cuda.synchronize()
    assert torch.equal(flux, flux2) and torch.equal(res_a, res_b) and not plan.status()
    lib.temxz_wave_destroy(h)
    lib.temxz_wave_destroy(None)


# ---- the operator of the averager ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_sph_wave_in_the_class_form_against_the_restatement(dtype):
    from pytemdiags_amd import sph_zonal_averager
    lat, lon, plev, f, L, ms, ref = case("ne4")
    lat_out = orc.zm_latitudes(1)
    Z = sph_zonal_averager(lat, lat_out, L, lon=lon, debug=False, wave_form="classes")
    Z.sph_compute_matrices()
    Zo = orc.ZonalAverager(lat, lat_out, L, mode="factorised")
    A = np.ascontiguousarray(np.asarray(f[1]).astype(dtype))
    A64 = A.astype(np.float64)
    for m in (1, 4):
        _, xc, xs = w.wave_fit(A64 - Zo.zonal_mean_native(A64), lat, lon, lat_out, m, L)
        gc, gs = Z.sph_wave(A, m)
        assert Z._waves[m].form == "classes" and gc.dtype == dtype and gc.shape == xc.shape
        e = fieldnorm_err(np.stack([gc, gs]), np.stack([xc, xs]))
        print("classes sph_wave %s m=%d: %.2e" % (np.dtype(dtype).name, m, e))
        assert e <= _tol(dtype), (m, e)
    bad = A.copy()
    bad[7, 0] = np.nan
    with pytest.raises(RuntimeError, match="has nans"):
        Z.sph_wave(bad, 1)
    assert not Z._plan.status() and np.all(np.isfinite(Z.sph_wave(A, 1)[0]))


# ---- stored bytes -----------------------------------------------------------------------------------------------------------------
def test_the_state_holds_fewer_bytes_than_the_generic_one():
    """ne8, L = 50, m = 1, right after creation: the generic state stores ncol x 100 x 8 bytes of basis (2.8 MB), the class
    form 16 bytes per entry of the row table, 10 x 7 x 128 bytes per class-group and the small matrices both keep."""
    from pytemdiags_amd import engine, synth, waves
    lat, lon = synth.cubed_sphere_gll(8)
    plan = engine.Plan(lat, orc.zm_latitudes(1), 50, device=0)
    try:
        gen, cls = waves.WaveState(plan, lon, (1,)), waves.WaveState(plan, lon, (1,), form="classes")
        try:
            print("ne8 L = 50 m = 1: generic state %d bytes, class form %d bytes" % (gen.workspace_bytes, cls.workspace_bytes))
            assert 0 < cls.workspace_bytes < gen.workspace_bytes
            assert gen.workspace_bytes >= lat.size * 100 * 8 and cls.workspace_bytes < lat.size * 100 * 8
        finally:
            gen.close()
            cls.close()
    finally:
        plan.close()
