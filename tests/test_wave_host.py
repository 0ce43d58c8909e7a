"""Zonal wavenumbers, host side: the ctypes table against pytemdiags_amd/include/temx_wave.h and the plain-C link check,
the refusals of the front end that are decided before any device call, and the host tables of the fit
(pytemdiags_amd/csrc/wave_tables.hpp, which needs no HIP) on their own under AddressSanitizer + UBSan: the normalised
recurrence of ``Pbar_l^m`` against ``scipy.special.lpmv``, the Kc / padding arithmetic, the argument checker's codes and
the Cholesky factor with its rank rule (a pivot at or below n 2^-52 of the largest diagonal entry is refused).  Needs no
GPU.

Bound of the recurrence: 1e-12 relative to the maximum of the row (one m, one latitude, l = m..255), at m in 1, 4, 32 and
latitudes that include +-89.9 degrees and the equator."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pytemdiags_amd", "include", "temx_wave.h")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
LATS = (-89.9, -60.0, -23.5, 0.0, 10.0, 45.0, 75.0, 89.9)


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_wave_header_declares_exactly_what_is_bound():
    from pytemdiags_amd import _lib, _wave
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(temxk_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _wave.SIGNATURES} == {
        "temxk_version", "temxk_wave_create", "temxk_wave_destroy", "temxk_wave_workspace_bytes", "temxk_wave_project",
        "temxk_wave_fluxes", "temxk_wave_status", "temxk_wave_shape", "temxk_wave_timing", "temxk_wave_timing_read"}
    assert not re.findall(r"\b(temx[vlicnmgw]?_[a-z0-9_]+)\s*\(", code)   # the other headers' ABI is not extended from here
    lib = _wave.load()
    assert lib is _lib.load() and lib.temxk_version() == _wave.WAVE_VERSION == 100
    for name, value in (("TEMXK_NF_MAX", _wave.NF_MAX), ("TEMXK_NM_MAX", _wave.NM_MAX), ("TEMXK_KC_MAX", _wave.KC_MAX)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const void*": C.c_void_p, "double*": C.c_void_p,
             "temxk_wave*": C.c_void_p, "const temxk_wave*": C.c_void_p, "temx_plan*": C.c_void_p,
             "temxk_wave**": C.POINTER(C.c_void_p), "const void* const*": C.POINTER(C.c_void_p),
             "const int*": C.POINTER(C.c_int), "const double*": C.POINTER(C.c_double), "int*": C.POINTER(C.c_int)}
    sig = dict((n, (r, a)) for n, r, a in _wave.SIGNATURES)
    names = {"temxk_wave_create": ["out", "plan", "lon_deg_host", "nm", "m_host"],
             "temxk_wave_project": ["wave", "mi", "nf", "fields_host", "dtype_host", "D", "parts", "coef_or_null", "stream"],
             "temxk_wave_fluxes": ["wave", "ua", "va", "ta", "wap", "dtype", "flux", "parts_or_null", "stream"],
             "temxk_wave_status": ["wave", "nonfinite_host", "stream"], "temxk_wave_shape": ["L", "m", "shape6_host"],
             "temxk_wave_timing": ["wave", "enable"], "temxk_wave_timing_read": ["wave", "sum_ms_host", "launches_host"]}
    for fn, want in names.items():
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert sig[fn] == (C.c_int, [ctype[p.rsplit(" ", 1)[0]] for p in params]), fn
        assert [p.rsplit(" ", 1)[1] for p in params] == want, fn
    assert sig["temxk_version"] == (C.c_int, []) and sig["temxk_wave_destroy"] == (None, [C.c_void_p])
    assert sig["temxk_wave_workspace_bytes"] == (C.c_int64, [C.c_void_p])
    # the entry points are function-try-blocks, like every other one; the other versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    for fn in names:
        assert re.search(r"^int %s\([^;{]*\)\s*try \{\s*$" % fn, src, re.M), fn
    for fn, v in (("temx", 402), ("temxv", 100), ("temxl", 100), ("temxi", 100), ("temxc", 100), ("temxm", 100),
                  ("temxn", 100), ("temxg", 100), ("temxw", 100), ("temxk", 100)):
        assert "int %s_version(void) { return %d; }" % (fn, v) in src, fn
    # the other nine headers declare nothing of this feature; the Makefile knows the new one
    for d in (os.path.join(ROOT, "include"), os.path.dirname(HEADER)):
        for n in os.listdir(d):
            if n != "temx_wave.h":
                assert "temxk_" not in open(os.path.join(d, n)).read(), n
    mk = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "Makefile")).read()
    assert "../include/temx_wave.h" in mk
    # the shapes come from the library (temxk_wave_shape = wave_shape of the header of the tables, which needs no HIP)
    hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "wave_tables.hpp")).read()
    assert hpp.count("IntList<4, 8, 16, 25, 32>") == 1 and "WAVE_SLICE_TB = 32" in hpp
    assert "WAVE_KC_MAX = %d" % _wave.KC_MAX in hpp and not re.search(r"#include\s*<hip", hpp)
    assert _wave.shape(50, 1) == dict(ndeg=50, Kc=100, nslice=1, tb_last=25, gstride=25, kpad=100)
    assert _wave.shape(20, 20) == dict(ndeg=1, Kc=2, nslice=1, tb_last=4, gstride=4, kpad=16)
    assert _wave.shape(255, 1) == dict(ndeg=255, Kc=510, nslice=4, tb_last=32, gstride=128, kpad=512)
    assert _wave.shape(99, 1)["nslice"] == 2 and _wave.shape(99, 1)["gstride"] == 32 + 25
    assert _wave.shape(60, 1)["tb_last"] == 32 and _wave.shape(70, 1) == dict(ndeg=70, Kc=140, nslice=2, tb_last=4, gstride=36, kpad=144)
    for L, m in ((0, 1), (512, 1), (10, 0), (10, 11)):
        out = (C.c_int * 6)()
        assert lib.temxk_wave_shape(L, m, out) == -1 and b"L must lie" in lib.temx_last_error()
    assert lib.temxk_wave_shape(10, 1, None) == -1 and lib.temxk_wave_status(None, None, None) == -1


def test_wave_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_wave")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_wave.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxk_version=100 create_rc=-1 project_rc=-1 fluxes_rc=-1 bytes=0" in out.stdout
    assert "temx_version=402" in out.stdout


# ---- wave_tables.hpp on its own, under the sanitizers ------------------------------------------------------------------
_program = {}


def _tables_output(tmp_path_factory):
    """tests/host/wave_tables_main.cpp built once with the host compiler under the sanitizers, and its output."""
    if "out" not in _program:
        if shutil.which("g++") is None:
            pytest.skip("no g++")
        if os.environ.get("LD_PRELOAD"):
            pytest.skip("AddressSanitizer does not start behind another preloaded library")
        exe = str(tmp_path_factory.mktemp("wave_tables") / "wave_tables_main")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                        os.path.join(ROOT, "tests", "host", "wave_tables_main.cpp"), "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        _program["out"] = out.stdout
    return _program["out"]


def _rows(stdout, j):
    """{m: Pbar_l^m, l = m..255} the program printed for latitude ``LATS[j]``."""
    rows = {}
    for line in stdout.splitlines():
        parts = line.split()
        if parts and parts[0] == "P" and int(parts[2]) == j:
            rows[int(parts[1])] = np.array(parts[3:], dtype=np.float64)
    assert sorted(rows) == [1, 4, 32] and all(v.size == 256 - m for m, v in rows.items())
    return rows


def test_wave_tables_shapes_checker_and_cholesky(tmp_path_factory):
    m = re.search(r"shapes=(\d+) refusals=(\d+) cholesky=ok", _tables_output(tmp_path_factory))
    assert m
    assert int(m.group(1)) == 511 * 512 // 2 and int(m.group(2)) == 10


def test_wave_tables_rank_rule(tmp_path_factory):
    """``wave_cholesky`` refuses a pivot at or below n 2^-52 max_j G[j][j]: the program's own checks (a positive definite
    5 x 5 matrix with row and column r scaled by 1e-14 is refused at pivot r, for every r, although the textbook
    recurrence finds that pivot positive; the same matrix times 1e-30 overall is accepted and inverted; the factor of
    every accepted matrix is the textbook one bit for bit; diag(1, t) is refused at t = 2 * 2^-52 and accepted one ulp
    above), and the rule restated here on the Nyquist basis of the 12 x 16 grid, whose numbers the rule was made for."""
    out = _tables_output(tmp_path_factory)
    assert "FAILED" not in out and re.search(r"cholesky=ok rank=ok\s*$", out)
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "wave_tables.hpp")).read()
    assert "(double)n * 0x1p-52 * dmax" in src and "if (!(s > least) || !std::isfinite(s)) return 1 + i;" in src
    # the numbers of the rule, in numpy: smallest pivot over largest diagonal entry of Ym^T Ym
    scipy_special = pytest.importorskip("scipy.special")
    from pytemdiags_amd import synth

    def ratio(nlat, nlon, L, mm):
        lat, lon = synth.latlon_grid(nlat, nlon)
        l = np.arange(mm, L + 1)
        norm = np.sqrt(2.0) * np.sqrt((2 * l + 1) / (4 * np.pi)
                                      * np.exp(scipy_special.gammaln(l - mm + 1) - scipy_special.gammaln(l + mm + 1)))
        P = norm[None, :] * scipy_special.lpmv(mm, l[None, :], np.sin(np.deg2rad(lat))[:, None])
        lam = np.deg2rad(lon)[:, None]
        Y = np.concatenate([P * np.cos(mm * lam), P * np.sin(mm * lam)], axis=1)
        G = Y.T @ Y
        n, F = G.shape[0], np.zeros_like(G)
        piv = []
        for i in range(n):
            for j in range(i + 1):
                s = G[i, j] - F[i, :j] @ F[j, :j]
                if i == j:
                    piv.append(s)
                    F[i, i] = np.sqrt(abs(s))
                else:
                    F[i, j] = s / F[j, j]
        return min(piv) / G.diagonal().max(), n * 2.0 ** -52

    for nlat, nlon, L, mm, refused in ((12, 16, 8, 8, True), (12, 16, 8, 7, False), (32, 48, 24, 24, True),
                                       (32, 48, 24, 23, False), (24, 48, 24, 1, False)):
        r, bound = ratio(nlat, nlon, L, mm)
        print("%d x %d L = %d m = %d: smallest pivot / largest diagonal %.2e (bound %.2e)" % (nlat, nlon, L, mm, r, bound))
        assert (r <= bound) == refused and (r < 1e-12 * bound if refused else r > 0.2), (nlat, nlon, L, mm, r)


@pytest.mark.parametrize("j", range(len(LATS)), ids=["lat%+.1f" % a for a in LATS])
def test_wave_tables_recurrence_against_scipy(j, tmp_path_factory):
    """``Pbar_l^m`` for m in 1, 4, 32 and l up to 255 against ``scipy.special.lpmv`` with the header's normalisation, within
    1e-12 of the row maximum.

    The header seeds the recurrence with cos(lat) = sqrt(1 - x^2), as ``lpmv`` does, so the two agree at the poles too
    (measured: 2.0e-13 at worst, at +-89.9 degrees and m = 1)."""
    scipy_special = pytest.importorskip("scipy.special")
    L = 255
    x = np.sin(np.deg2rad(LATS[j]))
    for mm, got in _rows(_tables_output(tmp_path_factory), j).items():
        l = np.arange(mm, L + 1)
        norm = np.sqrt(2.0) * np.sqrt((2 * l + 1) / (4 * np.pi)
                                      * np.exp(scipy_special.gammaln(l - mm + 1) - scipy_special.gammaln(l + mm + 1)))
        want = norm * scipy_special.lpmv(mm, l, x)
        assert np.all(np.isfinite(want)) and np.max(np.abs(want)) > 0
        e = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print("Pbar_l^%d at %+.1f degrees against scipy: %.2e of the row maximum" % (mm, LATS[j], e))
        assert e <= 1e-12, (mm, LATS[j], e)


@pytest.mark.parametrize("j", range(len(LATS)), ids=["lat%+.1f" % a for a in LATS])
def test_wave_tables_recurrence_against_extended_precision(j, tmp_path_factory):
    """The same rows against the recurrence of the contract evaluated with 60 digits from the same two doubles, x and
    1 - x^2 (cos^2 of the latitude as the header and ``lpmv`` form it): 1e-12 of the row maximum at every latitude.  This
    holds the normalisation, cos^m and the three-term recurrence in l to exact arithmetic (measured: 5.3e-14 at worst).
    What it leaves out on purpose is the rounding of 1 - x^2 itself, which the contract shares with ``lpmv``: with the
    exact 1 - x^2 of the same x the rows at +-89.9 degrees differ by 3.0e-12 (m = 1), 1.2e-11 (m = 4) and 9.4e-11
    (m = 32) of their maximum, for this header and for ``lpmv`` alike, and by at most 1.9e-14 at the other latitudes."""
    mp = pytest.importorskip("mpmath")
    L = 255
    with mp.workdps(60):
        xd = float(np.sin(np.deg2rad(LATS[j])))
        x = mp.mpf(xd)
        c = mp.sqrt(mp.mpf(1.0 - xd * xd))
        for mm, got in _rows(_tables_output(tmp_path_factory), j).items():
            r = mp.mpf(2 * mm + 1) / (4 * mp.pi)
            for k in range(1, mm + 1):
                r *= mp.mpf(2 * k - 1) / (2 * k)
            p2 = (-1) ** mm * mp.sqrt(2) * mp.sqrt(r) * c ** mm
            p1 = mp.sqrt(2 * mm + 3) * x * p2
            want = [p2, p1]
            for l in range(mm + 2, L + 1):
                a = mp.sqrt(mp.mpf(4 * l * l - 1) / (l * l - mm * mm))
                b = mp.sqrt(mp.mpf((l - 1) ** 2 - mm * mm) / (4 * (l - 1) ** 2 - 1))
                p2, p1 = p1, a * (x * p1 - b * p2)
                want.append(p1)
            want = np.array([float(v) for v in want])
            e = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            print("Pbar_l^%d at %+.1f degrees against 60 digits: %.2e of the row maximum" % (mm, LATS[j], e))
            assert e <= 1e-12, (mm, LATS[j], e)


# ---- front-end refusals before the device -------------------------------------------------------------------------------
def _tiny(nt=4):
    la = -90 + (np.arange(6) + 0.5) * 30.0
    lat = np.repeat(la, 8)
    lon = np.tile(np.arange(8) * 45.0, 6)
    plev = np.array([100.0, 500.0, 1000.0])
    return lat, lon, plev, np.zeros((lat.size, 3, nt))


BAD = [
    (dict(wavenumbers=(1, 2)), "needs lon="),
    (dict(wavenumbers=(1, 2), lon="short"), "lon has 47 entries"),
    (dict(wavenumbers=(1, 2), lon="nan"), "lon must be finite"),
    (dict(wavenumbers=(), lon="ok"), "empty"),
    (dict(wavenumbers=(0,), lon="ok"), "not in 1..L"),
    (dict(wavenumbers=(11,), lon="ok"), "not in 1..L"),
    (dict(wavenumbers=(1.0,), lon="ok"), "integers"),
    (dict(wavenumbers=(True,), lon="ok"), "integers"),
    (dict(wavenumbers=("2",), lon="ok"), "integers"),
    (dict(wavenumbers=(2, 3, 2), lon="ok"), "given twice"),
    (dict(wavenumbers=(1,), lon="ok", missing="mask"), "missing='mask'"),
    (dict(wavenumbers=(1,), lon="ok", lat_bins=True), "lat_bins"),
    (dict(wavenumbers=(1,), lon="ok", time_block=2), "time_block"),
    (dict(wavenumbers=(1,), lon="ok", climatology=True), "climatology"),
]


@pytest.mark.parametrize("kw,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_wave_keywords_are_refused_before_device(kw, match):
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f = _tiny()
    kw = dict(kw)
    if "lon" in kw:
        kw["lon"] = {"ok": lon, "short": lon[:-1], "nan": np.where(np.arange(lon.size) == 3, np.nan, lon)}[kw["lon"]]
    with pytest.raises(ValueError, match=match):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, L=10, device=99, **kw)
    with pytest.raises(ValueError, match=match):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=plev, ps=np.zeros((lat.size, 4)), hyam=np.zeros(3),
                                         hybm=np.ones(3), L=10, device=99, **kw)


def test_wave_keywords_are_keyword_only_and_off_by_default():
    import inspect
    from pytemdiags_amd import TEMDiagnostics, sph_zonal_averager, waves
    for name in ("lon", "wavenumbers"):
        p = inspect.signature(TEMDiagnostics.__init__).parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, name
    p = inspect.signature(sph_zonal_averager.__init__).parameters["lon"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert waves.check_wavenumbers([3, np.int64(1)], 5) == (3, 1) and waves.check_wavenumbers(2, 5) == (2,)
    assert issubclass(waves.WaveSet, __import__("pytemdiags_amd").climatology.ResultSet)
    assert waves.FIELD_NAMES == ("ua", "va", "theta", "wap")


def test_sph_wave_refusals_need_no_device():
    from pytemdiags_amd import sph_zonal_averager
    lat, lon, _, f = _tiny()
    lat_out = np.arange(-85.0, 90.0, 10.0)
    A = f[:, 0, :]
    with pytest.raises(ValueError, match="lon has 47 entries"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon[:-1], device=99)
    with pytest.raises(ValueError, match="needs lon="):
        sph_zonal_averager(lat, lat_out, 4, device=99).sph_wave(A, 1)
    with pytest.raises(ValueError, match="weights averager"):
        sph_zonal_averager(lat, lat_out, 4, weights=np.full(lat.size, 1.0 / lat.size), lon=lon, device=99).sph_wave(A, 1)
    with pytest.raises(ValueError, match="missing='mask'"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon, missing="mask", device=99).sph_wave(A, 1)
    with pytest.raises(ValueError, match="lat_bins"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon, lat_bins=True, device=99).sph_wave(A, 1)
    for bad in (0, 5, 1.5, "1"):
        with pytest.raises(ValueError):
            sph_zonal_averager(lat, lat_out, 4, lon=lon, device=99).sph_wave(A, bad)
    # no plan yet: the reference's message, as for sph_zonal_mean
    with pytest.raises(RuntimeError, match="sph_compute_matrices"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon, device=99).sph_wave(A, 1)
