"""Model levels to pressure levels, the part that needs no GPU: the numpy restatement of the contract of
include/temx_vert.h (``interp_ref``, which test_gpu_vertical.py compares the kernels against), the fixtures both
files share, self-checks of that reference, the validation errors raised before any device work, and the header,
the ctypes table and a plain-C consumer of the second header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 37 standard pressure levels [hPa]
PLEV37 = np.array([1, 2, 3, 5, 7, 10, 20, 30, 50, 70, 100, 125, 150, 175, 200, 225, 250, 300, 350, 400, 450, 500, 550,
                   600, 650, 700, 750, 775, 800, 825, 850, 875, 900, 925, 950, 975, 1000], dtype=np.float64)


def interp_ref(f, p, plev_pa, method="log", edge="nan", psurf=None):
    """The contract, per (column, time): np.interp over ln p or p inside [p_top, p_bot]; outside, NaN or (edge="hold")
    the top value above p_top and the bottom value between p_bot and the surface psurf [ncol][nt] (None: the surface
    is p_bot, nothing below is held); a column whose pressures are not finite and strictly increasing is NaN.
    f, p: [ncol][nlev][nt]; everything in fp64."""
    f = np.asarray(f, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    pt = np.asarray(plev_pa, dtype=np.float64)
    ncol, nlev, nt = f.shape
    surf = p[:, -1, :] if psurf is None else np.asarray(psurf, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.log(p) if method == "log" else p
        xt = np.log(pt) if method == "log" else pt
        good = np.all(np.isfinite(p), axis=1) & np.isfinite(surf) & np.all(np.diff(p, axis=1) > 0, axis=1)   # [ncol][nt]
        above = pt[None, :, None] < p[:, :1, :]
        below = pt[None, :, None] > p[:, -1:, :]
        held = below & (pt[None, :, None] <= surf[:, None, :])
    out = np.full((ncol, pt.size, nt), np.nan)
    for i in range(ncol):
        for t in range(nt):
            if good[i, t]:
                out[i, :, t] = np.interp(xt, x[i, :, t], f[i, :, t])
    out[above | below] = np.nan
    if edge == "hold":
        out = np.where(above, f[:, :1, :], out)
        out = np.where(held, f[:, -1:, :], out)
    out[np.broadcast_to(~good[:, None, :], out.shape)] = np.nan
    return out


def hybrid_levels(nlev=72):
    """Hybrid coefficients of a model with its top at 0.1 hPa: pure pressure above eta = 0.2, terrain following below."""
    eta = np.exp(np.linspace(np.log(1e-4), np.log(0.9976), nlev))
    b = np.maximum((eta - 0.2) / 0.8, 0.0) ** 1.3
    return eta - b, b


def surface_pressure(lat, lon, nt):
    """The surface of test_missing_host.surface_mask, in Pa: 1e5 +- 1500, a southern polar cap at 6.5e4, a plateau at
    6e4.  [ncol][nt]."""
    lat = np.asarray(lat)[:, None]
    lon = np.asarray(lon)[:, None]
    t = np.arange(nt)[None, :]
    ps = 1000.0 + 15.0 * np.sin(np.deg2rad(lon) + 0.7 * t) * np.cos(np.deg2rad(lat))
    ps = np.where(lat < -70.0, 650.0, ps)
    plateau = (np.abs(lat - 33.0) < 8.0) & (np.abs(lon - 88.0) < 15.0)
    return np.where(plateau, 600.0, ps) * 100.0


def hybrid_pressure(hyam, hybm, ps, p0=1e5):
    return hyam[None, :, None] * p0 + hybm[None, :, None] * ps[:, None, :]


def model_fields(lat, lon, nlev, nt, n=4, seed=5, dtype=np.float64):
    """n smooth fields on nlev model levels (the analytic fields and tracers at the levels' nominal pressures)."""
    from pytemdiags_amd import synth
    nominal = np.exp(np.linspace(np.log(0.1), np.log(997.6), nlev))
    fs = list(synth.analytic_fields(lat, lon, nominal, nt, seed=seed))
    fs += [synth.analytic_tracer(lat, lon, nominal, nt, which=i % 2, seed=100 + i) for i in range(max(0, n - 4))]
    return [np.ascontiguousarray(x.astype(dtype)) for x in fs[:n]]


def atmosphere_on_model_levels(lat, lon, p, nt, seed=3, dtype=np.float64):
    """ua, va, ta, wap of one atmosphere sampled on model levels: the analytic fields evaluated at each point's own
    pressure p [ncol][nlev][nt] in Pa, so that what the interpolation returns is that atmosphere on pressure levels.
    (model_fields places the profiles at nominal pressures whatever the surface pressure is.  That suits the kernel
    tests, which only need smooth numbers, but over the plateau and the polar cap it squeezes the whole profile above
    600 hPa; the zonal mean d(theta)/dp the TEM formulas divide by then comes close to zero on the lowest levels, and
    the oracle itself moves by 5e-11 (vtem, field-normalised) when its inputs move by 1e-15, against 2e-13 for the
    pressure-level fields the pipeline's 1e-10 parity tolerance was set on: test_frontend_fixture_is_well_conditioned.)"""
    from pytemdiags_amd import synth
    return [np.ascontiguousarray(x) for x in synth.analytic_fields(lat, lon, p / 100.0, nt, seed=seed, dtype=dtype)]


def frontend_case(nt=2, nlev=72, dtype=np.float64):
    """The ne8 fixture with an atmosphere that is consistent with its surface pressure."""
    lat, lon, hyam, hybm, ps = case_ne8(nt=nt, nlev=nlev)
    f = atmosphere_on_model_levels(lat, lon, hybrid_pressure(hyam, hybm, ps), nt, dtype=dtype)
    return lat, lon, hyam, hybm, ps, f


def inside_everywhere(p, plev_pa):
    """Target levels that lie inside every column."""
    return (plev_pa >= p[:, 0, :].max()) & (plev_pa <= p[:, -1, :].min())


def assert_no_edge_ties(p, plev_pa):
    """A condition on the inputs: no target within 1e-9 (in ln p) of a column's first or last level, so the NaN
    pattern has no rounding ties and a GPU test may demand identical patterns with nothing excluded.  (The surface
    needs no such margin: a target is compared with ps itself, which both sides hold exactly.)"""
    lt = np.log(plev_pa)[None, :, None]
    for edge in (p[:, :1, :], p[:, -1:, :]):
        assert np.min(np.abs(lt - np.log(edge))) > 1e-9


def case_ne8(nt=3, nlev=72):
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(8)
    hyam, hybm = hybrid_levels(nlev)
    ps = surface_pressure(lat, lon, nt)
    return lat, lon, hyam, hybm, ps


# ---- the fixtures are what the GPU tests assume -------------------------------------------------------------------
def test_fixture_has_no_target_on_a_column_edge():
    """The shapes the GPU tests run: no edge ties, a few per cent of the targets below ground, 23 levels inside every
    column, and the amplification ln p / d ln p the fp64 tolerance is derived from."""
    for nlev, nt in ((72, 3), (128, 3), (72, 91), (128, 30)):
        lat, lon, hyam, hybm, ps = case_ne8(nt=nt, nlev=nlev)
        p = hybrid_pressure(hyam, hybm, ps)
        assert np.all(np.diff(p, axis=1) > 0)
        assert_no_edge_ties(p, PLEV37 * 100.0)
        outside = (PLEV37[None, :, None] * 100.0 > p[:, -1:, :]) | (PLEV37[None, :, None] * 100.0 < p[:, :1, :])
        assert 0.01 < outside.mean() < 0.10                       # a few per cent of the targets are below ground
        assert int(inside_everywhere(p, PLEV37 * 100.0).sum()) == 23
        x = np.log(p)
        assert np.max(x[:, 1:, :] / np.diff(x, axis=1)) < 300      # the amplification the fp64 tolerance is derived from


def test_frontend_fixture_is_well_conditioned():
    """A condition on the inputs of the end-to-end test against the oracle, checked on the oracle alone.  Two correct
    interpolations differ by roundings (the kernel and np.interp do not take the same logarithms or blend in the same
    order), about 1e-15 of a value.  The 1e-10 tolerance of the pipeline can only be asked of what comes after if such a
    difference in the fields moves the oracle's own results by far less: at most 1e-12, a hundredth of it.  (The
    pressure-level fields the tolerance was set on move by 2e-13; these move by about as much.)"""
    from conftest import fieldnorm_err
    from oracle import tem_oracle as orc
    lat, lon, hyam, hybm, ps, f = frontend_case()
    p = hybrid_pressure(hyam, hybm, ps)
    levels = PLEV37[inside_everywhere(p, PLEV37 * 100.0)]
    g = [interp_ref(x, p, levels * 100.0, psurf=ps) for x in f]
    rng = np.random.default_rng(0)
    moved = [x * (1.0 + 1e-15 * rng.uniform(-1.0, 1.0, x.shape)) for x in g]
    a = orc.TEMOracle(*g, lat, levels, L=30, mode="factorised")
    b = orc.TEMOracle(*moved, lat, levels, L=30, mode="factorised")
    for n in ("vtem", "omegatem", "wtem", "psitem", "epfy", "epfz", "epdiv", "utendepfd", "utendvtem", "utendwtem"):
        e = fieldnorm_err(getattr(b, n)(), getattr(a, n)())
        print("%s: %.3e" % (n, e))
        assert e <= 1e-12, (n, e)


# ---- self-checks of the reference ---------------------------------------------------------------------------------
def _small(nt=2, ncol=40):
    rng = np.random.default_rng(7)
    hyam, hybm = hybrid_levels(72)
    ps = rng.uniform(5.5e4, 1.03e5, (ncol, nt))
    return hyam, hybm, ps, hybrid_pressure(hyam, hybm, ps)


def test_reference_reproduces_a_field_linear_in_log_p():
    hyam, hybm, ps, p = _small()
    f = 3.0 - 2.5 * np.log(p)
    pt = PLEV37 * 100.0
    out = interp_ref(f, p, pt)
    want = np.broadcast_to((3.0 - 2.5 * np.log(pt))[None, :, None], out.shape)
    fin = np.isfinite(out)
    assert fin.any() and np.max(np.abs(out[fin] - want[fin])) <= 1e-13 * np.max(np.abs(want))
    lin = interp_ref(1.0 + 2e-4 * p, p, pt, method="linear")
    assert np.array_equal(np.isfinite(lin), fin)
    assert np.max(np.abs(lin[fin] - np.broadcast_to((1.0 + 2e-4 * pt)[None, :, None], out.shape)[fin])) <= 1e-13 * 21.0


def test_reference_hold_differs_from_nan_only_outside_the_column():
    hyam, hybm, ps, p = _small()
    rng = np.random.default_rng(1)
    f = rng.standard_normal(p.shape)
    pt = np.concatenate([[5.0], PLEV37 * 100.0])                  # 0.05 hPa: above the model top
    a = interp_ref(f, p, pt, edge="nan")
    h = interp_ref(f, p, pt, edge="hold", psurf=ps)
    inside = (pt[None, :, None] >= p[:, :1, :]) & (pt[None, :, None] <= p[:, -1:, :])
    assert np.array_equal(a[inside], h[inside]) and np.all(np.isfinite(a[inside])) and np.all(np.isnan(a[~inside]))
    assert np.array_equal(h[:, 0, :], f[:, 0, :])                 # held above the top
    between = (pt[None, :, None] > p[:, -1:, :]) & (pt[None, :, None] <= ps[:, None, :])
    below = pt[None, :, None] > ps[:, None, :]
    assert between.any() and below.any()
    assert np.array_equal(h[between], np.broadcast_to(f[:, -1:, :], h.shape)[between]) and np.all(np.isnan(h[below]))
    # field mode: the surface is the bottom level, nothing below it is held
    hf = interp_ref(f, p, pt, edge="hold")
    assert np.all(np.isnan(hf[pt[None, :, None] > p[:, -1:, :]]))


def test_reference_bad_columns_and_nan_values():
    hyam, hybm, ps, p = _small()
    f = np.random.default_rng(2).standard_normal(p.shape)
    pt = PLEV37 * 100.0
    good = interp_ref(f, p, pt)
    q = p.copy()
    q[3, 40, 1] = q[3, 39, 1]                                     # not strictly increasing
    q[5, 10, 0] = np.nan
    out = interp_ref(f, q, pt)
    assert np.all(np.isnan(out[3, :, 1])) and np.all(np.isnan(out[5, :, 0]))
    keep = np.ones(out.shape, bool)
    keep[3, :, 1] = keep[5, :, 0] = False
    assert np.array_equal(out[keep], good[keep], equal_nan=True)
    g = f.copy()
    g[7, 50, 0] = np.nan                                          # reaches the brackets (49, 50) and (50, 51) only
    out = interp_ref(g, p, pt)
    touched = (pt > p[7, 49, 0]) & (pt < p[7, 51, 0])
    assert touched.any() and np.all(np.isnan(out[7, touched, 0]))
    assert np.array_equal(out[7, ~touched, 0], good[7, ~touched, 0], equal_nan=True)


# ---- validation before any device call ----------------------------------------------------------------------------
def test_validation_errors_are_raised_without_a_device():
    from pytemdiags_amd import interp_to_pressure
    hyam, hybm = hybrid_levels(8)
    f = np.zeros((5, 8, 2))
    ps = np.full((5, 2), 1e5)
    ok = dict(ps=ps, hyam=hyam, hybm=hybm)
    with pytest.raises(ValueError, match="exactly one"):
        interp_to_pressure(f, [500.0], hyam=hyam, hybm=hybm)
    with pytest.raises(ValueError, match="exactly one"):
        interp_to_pressure(f, [500.0], p=np.zeros_like(f), **ok)
    with pytest.raises(ValueError, match="hyam"):
        interp_to_pressure(f, [500.0], ps=ps, hyam=hyam)
    with pytest.raises(ValueError, match="method"):
        interp_to_pressure(f, [500.0], method="cubic", **ok)
    with pytest.raises(ValueError, match="edge"):
        interp_to_pressure(f, [500.0], edge="extrapolate", **ok)
    with pytest.raises(ValueError, match="repeated"):
        interp_to_pressure(f, [500.0, 700.0, 700.0], **ok)
    with pytest.raises(ValueError, match="shape"):
        interp_to_pressure([f, np.zeros((5, 7, 2))], [500.0], **ok)
    with pytest.raises(ValueError, match="ps has shape"):
        interp_to_pressure(f, [500.0], ps=np.full((4, 2), 1e5), hyam=hyam, hybm=hybm)
    with pytest.raises(ValueError, match="p has shape"):
        interp_to_pressure(f, [500.0], p=np.zeros((5, 8, 3)))
    with pytest.raises(ValueError, match="levels"):
        interp_to_pressure(f, [500.0], ps=ps, hyam=hyam[:-1], hybm=hybm[:-1])
    # monotone at the largest surface pressure, not at the smallest: one reduction over ps finds it
    a = np.linspace(1e-3, 0.3, 8)
    b = np.array([0, 0, 0, 0, 0.1, 0.35, 0.55, 0.7])
    b[5], a[5] = 0.2, a[4] - 0.047                                # p_5 - p_4 = 0.1 ps - 0.047 p0 < 0 for ps < 4.7e4
    psv = np.full((5, 2), 1e5)
    psv[2, 1] = 3e4
    with pytest.raises(ValueError, match="not strictly increasing"):
        interp_to_pressure(f, [500.0], ps=psv, hyam=a, hybm=b)
    with pytest.raises(ValueError, match="not strictly increasing"):
        interp_to_pressure(f, [500.0], ps=ps, hyam=hyam[::-1], hybm=hybm[::-1])     # bottom first


def test_from_model_levels_validates_before_a_device():
    from pytemdiags_amd import TEMDiagnostics
    hyam, hybm = hybrid_levels(8)
    f = np.zeros((5, 8, 2))
    lat = np.linspace(-80, 80, 5)
    ps = np.full((5, 2), 1e5)
    with pytest.raises(ValueError, match="exactly one"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=[500.0], hyam=hyam, hybm=hybm)
    with pytest.raises(NotImplementedError, match="tracers"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=[500.0], ps=ps, hyam=hyam, hybm=hybm, q=f,
                                         missing="mask")
    with pytest.raises(ValueError, match="missing"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=[500.0], ps=ps, hyam=hyam, hybm=hybm, missing="bogus")


# ---- header, bindings, plain-C consumer ---------------------------------------------------------------------------
def test_vert_header_declares_exactly_what_is_bound():
    from pytemdiags_amd import _lib, _vert
    hdr = open(os.path.join(ROOT, "include", "temx_vert.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(temxv_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _vert.SIGNATURES}
    assert not re.findall(r"\b(temx_[a-z0-9_]+)\s*\(", code)      # the first header's ABI is not extended from here
    lib = _vert.load()
    assert lib is _lib.load() and lib.temxv_version() == _vert.VERT_VERSION == 100
    for name, value in (("TEMXV_P_HYBRID", _vert.P_HYBRID), ("TEMXV_P_FIELD", _vert.P_FIELD), ("TEMXV_LOG", _vert.LOG),
                        ("TEMXV_LINEAR", _vert.LINEAR), ("TEMXV_EDGE_NAN", _vert.EDGE_NAN),
                        ("TEMXV_EDGE_HOLD", _vert.EDGE_HOLD), ("TEMXV_NF_MAX", _vert.NF_MAX)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    # every temxv entry point with a body is a function-try-block, like the entry points of temx.h
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    assert re.search(r"^int temxv_interp\([^;{]*\)\s*try \{\s*$", src, re.M)


def test_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _vert
    lib = _vert.load()
    plev = (C.c_double * 2)(5e4, 7e4)
    bad_plev = (C.c_double * 2)(7e4, 5e4)
    hy = (C.c_double * 3)(0.1, 0.2, 0.3)
    src, dst = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(1 << 20)

    def call(nf=1, src=src, dst=dst, dtype=0, plev=plev, pmode=0, hyam=hy, hybm=hy, ps=C.c_void_p(1 << 24), method=0,
             edge=0):
        # device 99 does not exist: a call that got as far as the device would come back TEMX_EHIP, not TEMX_EINVAL
        return lib.temxv_interp(99, nf, src, dst, dtype, 4, 3, 2, 2, plev, pmode, hyam, hybm, 1e5, ps, 0, method, edge,
                                None)
    assert call(nf=0) == -1 and b"nf" in lib.temx_last_error()
    assert call(nf=9) == -1
    assert call(src=None) == -1 and call(dst=None) == -1 and call(plev=None) == -1 and call(ps=None) == -1
    assert call(hyam=None) == -1
    assert call(src=(C.c_void_p * 1)(None)) == -1
    assert call(plev=bad_plev) == -1 and call(plev=(C.c_double * 2)(-1.0, 5e4)) == -1
    assert call(dtype=2) == -1 and call(pmode=2) == -1 and call(method=2) == -1 and call(edge=-1) == -1
    assert call(dst=src) == -1 and b"overlaps" in lib.temx_last_error()
    assert call(dst=(C.c_void_p * 1)(4096 + 64)) == -1            # partial overlap is aliasing too
    assert call() == -2                                           # well-formed: only now is the device touched


def test_vert_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_vert")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_vert.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxv_version=100" in out.stdout and "nf0_rc=-1" in out.stdout
