"""The class form of the zonal-wavenumber fit, host side: the ctypes table against
pytemdiags_amd/include_wavecls/temx_wavecls.h and the plain-C link check, the host tables of the form
(pytemdiags_amd/csrc/wave_class_tables.hpp, which needs no HIP) on their own under AddressSanitizer + UBSan for every
grid of tests/test_gpu_wavecls.py, and the refusals of the front end that are decided before any device call.  Needs no
GPU."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a directory of its own: tests/test_tfilt_host.py pins the number of headers in the two include directories
HEADER = os.path.join(ROOT, "pytemdiags_amd", "include_wavecls", "temx_wavecls.h")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
ENTRY_POINTS = {"temxz_version", "temxz_wave_create", "temxz_wave_destroy", "temxz_wave_workspace_bytes",
                "temxz_wave_project", "temxz_wave_fluxes", "temxz_wave_status", "temxz_wave_shape", "temxz_wave_launch"}


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_wavecls_header_declares_exactly_what_is_bound():
    from pytemdiags_amd import _lib, _wavecls
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(temxz_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _wavecls.SIGNATURES} == ENTRY_POINTS
    # no other header's prefix anywhere in the text, comments included: the wave header is named by its file
    assert not re.findall(r"temx[vlicnmgwkf]_", text) and "temx_wave.h" in text
    lib = _wavecls.load()
    assert lib is _lib.load() and lib.temxz_version() == _wavecls.WAVECLS_VERSION == 100
    for name, value in (("TEMXZ_NF_MAX", _wavecls.NF_MAX), ("TEMXZ_NM_MAX", _wavecls.NM_MAX), ("TEMXZ_NDEG_MAX", _wavecls.NDEG_MAX)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const void*": C.c_void_p, "double*": C.c_void_p,
             "temxz_wave*": C.c_void_p, "const temxz_wave*": C.c_void_p, "temx_plan*": C.c_void_p,
             "temxz_wave**": C.POINTER(C.c_void_p), "const void* const*": C.POINTER(C.c_void_p),
             "const int*": C.POINTER(C.c_int), "const double*": C.POINTER(C.c_double), "int*": C.POINTER(C.c_int)}
    sig = dict((n, (r, a)) for n, r, a in _wavecls.SIGNATURES)
    names = {"temxz_wave_create": ["out", "plan", "lon_deg_host", "nm", "m_host"],
             "temxz_wave_project": ["wave", "mi", "nf", "fields_host", "dtype_host", "D", "parts", "coef_or_null", "stream"],
             "temxz_wave_fluxes": ["wave", "ua", "va", "ta", "wap", "dtype", "flux", "parts_or_null", "stream"],
             "temxz_wave_status": ["wave", "nonfinite_host", "stream"], "temxz_wave_shape": ["L", "m", "shape_host"],
             "temxz_wave_launch": ["wave", "mi", "nf", "D", "out_host"]}
    for fn, want in names.items():
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert sig[fn] == (C.c_int, [ctype[p.rsplit(" ", 1)[0]] for p in params]), fn
        assert [p.rsplit(" ", 1)[1] for p in params] == want, fn
    assert sig["temxz_version"] == (C.c_int, []) and sig["temxz_wave_destroy"] == (None, [C.c_void_p])
    assert sig["temxz_wave_workspace_bytes"] == (C.c_int64, [C.c_void_p])
    # the calls mirror the generic ones argument for argument
    from pytemdiags_amd import _wave
    gen = dict((n, (r, a)) for n, r, a in _wave.SIGNATURES)
    for fn in ("create", "destroy", "workspace_bytes", "project", "fluxes", "status"):
        assert sig["temxz_wave_" + fn] == gen["temxk_wave_" + fn], fn
    # the entry points are function-try-blocks, like every other one; the other versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    for fn in names:
        assert re.search(r"^int %s\([^;{]*\)\s*try \{\s*$" % fn, src, re.M), fn
    for fn, v in (("temx", 402), ("temxv", 100), ("temxl", 100), ("temxi", 100), ("temxc", 100), ("temxm", 100),
                  ("temxn", 100), ("temxg", 100), ("temxw", 100), ("temxk", 100), ("temxf", 100), ("temxz", 100)):
        assert "int %s_version(void) { return %d; }" % (fn, v) in src, fn
    # the other eleven headers declare nothing of this feature; the Makefile knows the new one
    assert os.listdir(os.path.dirname(HEADER)) == ["temx_wavecls.h"]
    seen = 0
    for d in (os.path.join(ROOT, "include"), os.path.join(ROOT, "pytemdiags_amd", "include")):
        for n in os.listdir(d):
            seen += 1
            assert "temxz_" not in open(os.path.join(d, n)).read(), n
    assert seen == 11
    mk = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "Makefile")).read()
    assert "../include_wavecls/temx_wavecls.h" in mk
    # the shapes come from the library (wavecls_shape of the header of the tables, which needs no HIP)
    hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "wave_class_tables.hpp")).read()
    assert hpp.count("IntList<2, 4, 7, 8>") == 1 and "WAVECLS_NDEG_MAX = %d" % _wavecls.NDEG_MAX in hpp
    assert not re.search(r"#include\s*<hip", hpp)
    assert _wavecls.shape(50, 1) == dict(ndeg=50, Kc=100, TBS=7, nacc=28, fpw=1)
    assert _wavecls.shape(50, 3) == dict(ndeg=48, Kc=96, TBS=7, nacc=28, fpw=1)
    assert _wavecls.shape(20, 20) == dict(ndeg=1, Kc=2, TBS=2, nacc=8, fpw=1)
    assert _wavecls.shape(20, 1)["TBS"] == 4 and _wavecls.shape(12, 4)["TBS"] == 2 and _wavecls.shape(64, 1)["TBS"] == 8
    assert _wavecls.shape(511, 448)["ndeg"] == 64
    out = (C.c_int * 5)()
    for L, m in ((0, 1), (512, 1), (10, 0), (10, 11)):
        assert lib.temxz_wave_shape(L, m, out) == -1 and b"L must lie" in lib.temx_last_error()
    assert lib.temxz_wave_shape(65, 1, out) == -6 and b"65 degrees" in lib.temx_last_error()
    assert lib.temxz_wave_shape(10, 1, None) == -1 and lib.temxz_wave_status(None, None, None) == -1
    assert lib.temxz_wave_launch(None, 0, 4, 8, (C.c_int * 4)()) == -1


def test_wavecls_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_wavecls")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_wavecls.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxz_version=100 create_rc=-1 project_rc=-1 fluxes_rc=-1 bytes=0 shape=50,100,7,28,1" in out.stdout
    assert "temx_version=402" in out.stdout


# ---- wave_class_tables.hpp on its own, under the sanitizers ----------------------------------------------------------
_program = {}
# (grid, side cap of an fp32 plan, wavenumbers): every row table tests/test_gpu_wavecls.py sweeps
TABLES = [("ne4", 0, (1, 2, 4)), ("ne8", 0, (1, 3, 20)), ("latlon24x48", 0, (1, 4, 10)), ("latlon24x48", 8, (1, 4, 10)),
          ("ne8", 8, (1,))]


def _grid(name):
    from pytemdiags_amd import synth
    return synth.latlon_grid(24, 48) if name == "latlon24x48" else synth.cubed_sphere_gll(int(name[2:]))


def _exe(tmp_path_factory):
    """tests/host/wave_class_tables_main.cpp built once with the host compiler under the sanitizers."""
    if "exe" not in _program:
        if shutil.which("g++") is None:
            pytest.skip("no g++")
        if os.environ.get("LD_PRELOAD"):
            pytest.skip("AddressSanitizer does not start behind another preloaded library")
        d = tmp_path_factory.mktemp("wave_class_tables")
        exe = str(d / "wave_class_tables_main")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                        os.path.join(ROOT, "tests", "host", "wave_class_tables_main.cpp"), "-o", exe], check=True)
        _program["exe"], _program["dir"] = exe, d
    return _program["exe"], _program["dir"]


@pytest.mark.parametrize("grid,cap,ms", TABLES, ids=["%s-cap%d" % (g, c) for g, c, _ in TABLES])
def test_wave_class_tables_weights_representatives_layout(grid, cap, ms, tmp_path_factory):
    """Every member entry carries the weights of its own longitude, padding carries zeros, each class side has exactly
    one representative, the block layout round-trips, the shapes and the count of cuts inside a group hold: the
    program's own checks.  Here: the sides the suite means to meet are there."""
    exe, d = _exe(tmp_path_factory)
    lat, lon = _grid(grid)
    path = str(d / ("%s.txt" % grid))
    if not os.path.exists(path):
        with open(path, "w") as fh:
            fh.write("%d\n" % len(lat))
            fh.writelines("%.17g %.17g\n" % (a, b) for a, b in zip(lat, lon))
    out = subprocess.run([exe, path, str(cap)] + [str(m) for m in ms], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "FAILED" not in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"N=(\d+) classes=(\d+) groups=(\d+) batches=(\d+) max_side=(\d+) weights=ok reps=ok layout=ok shapes=(\d+) cuts=ok\s*$",
                  out.stdout)
    assert m, out.stdout
    N, ncls, groups, batches, max_side, shapes = (int(v) for v in m.groups())
    print("%s cap %d: %d columns, %d classes in %d groups, %d batches, longest side %d" % (grid, cap, N, ncls, groups, batches, max_side))
    assert N == len(lat) and groups == (ncls + 3) // 4
    # (L, m) with at most 64 degrees: 64 per L beyond 64, all of them below
    assert shapes == sum(min(L, 64) for L in range(1, 512))
    if grid == "latlon24x48":
        # 12 classes of 48 + 48 (twelve batches per side), or the same sides cut into parts of 8: 72 classes at 12 latitudes
        assert (ncls, max_side, batches) == ((12, 48, 72) if cap == 0 else (72, 8, 72))
    else:
        assert max_side >= 8 and ncls > 60


# ---- front-end refusals before the device -------------------------------------------------------------------------------
def _tiny(nt=4):
    la = -90 + (np.arange(6) + 0.5) * 30.0
    lat = np.repeat(la, 8)
    lon = np.tile(np.arange(8) * 45.0, 6)
    plev = np.array([100.0, 500.0, 1000.0])
    return lat, lon, plev, np.zeros((lat.size, 3, nt))


BAD = [
    (dict(wave_form="classes"), "needs wavenumbers="),
    (dict(wave_form="class", wavenumbers=(1,), lon="ok"), "wave_form must be one of"),
    (dict(wave_form="class"), "wave_form must be one of"),
    (dict(wave_form=None, wavenumbers=(1,), lon="ok"), "wave_form must be one of"),
    (dict(wave_form=1), "wave_form must be one of"),
    (dict(wave_form="classes", wavenumbers=(1, 2)), "needs lon="),
    (dict(wave_form="classes", wavenumbers=(1, 2), lon="short"), "lon has 47 entries"),
    (dict(wave_form="classes", wavenumbers=(1, 2), lon="nan"), "lon must be finite"),
    (dict(wave_form="classes", wavenumbers=(), lon="ok"), "empty"),
    (dict(wave_form="classes", wavenumbers=(0,), lon="ok"), "not in 1..L"),
    (dict(wave_form="classes", wavenumbers=(11,), lon="ok"), "not in 1..L"),
    (dict(wave_form="classes", wavenumbers=(1.0,), lon="ok"), "integers"),
    (dict(wave_form="classes", wavenumbers=(2, 3, 2), lon="ok"), "given twice"),
    (dict(wave_form="classes", wavenumbers=(1,), lon="ok", missing="mask"), "missing='mask'"),
    (dict(wave_form="classes", wavenumbers=(1,), lon="ok", lat_bins=True), "lat_bins"),
    (dict(wave_form="classes", wavenumbers=(1,), lon="ok", time_block=2), "time_block"),
    (dict(wave_form="classes", wavenumbers=(1,), lon="ok", climatology=True), "climatology"),
]


@pytest.mark.parametrize("kw,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_wave_form_keywords_are_refused_before_device(kw, match):
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


def test_wave_form_is_keyword_only_and_generic_by_default():
    from pytemdiags_amd import TEMDiagnostics, sph_zonal_averager, waves
    for cls in (TEMDiagnostics, sph_zonal_averager):
        p = inspect.signature(cls.__init__).parameters["wave_form"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "generic", cls
    assert inspect.signature(waves.WaveState.__init__).parameters["form"].default == "generic"
    assert waves.WAVE_FORMS == ("generic", "classes")
    assert waves.check_form("generic", False) == "generic" and waves.check_form("classes") == "classes"


def test_sph_wave_form_refusals_need_no_device():
    from pytemdiags_amd import sph_zonal_averager
    lat, lon, _, f = _tiny()
    lat_out = np.arange(-85.0, 90.0, 10.0)
    A = f[:, 0, :]
    with pytest.raises(ValueError, match="wave_form must be one of"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon, wave_form="fast", device=99)
    with pytest.raises(ValueError, match="needs lon="):
        sph_zonal_averager(lat, lat_out, 4, wave_form="classes", device=99)
    with pytest.raises(ValueError, match="lon has 47 entries"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon[:-1], wave_form="classes", device=99)
    with pytest.raises(ValueError, match="weights averager"):
        sph_zonal_averager(lat, lat_out, 4, weights=np.full(lat.size, 1.0 / lat.size), lon=lon, wave_form="classes",
                           device=99).sph_wave(A, 1)
    with pytest.raises(ValueError, match="missing='mask'"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon, missing="mask", wave_form="classes", device=99).sph_wave(A, 1)
    with pytest.raises(ValueError, match="lat_bins"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon, lat_bins=True, wave_form="classes", device=99).sph_wave(A, 1)
    for bad in (0, 5, 1.5, "1"):
        with pytest.raises(ValueError):
            sph_zonal_averager(lat, lat_out, 4, lon=lon, wave_form="classes", device=99).sph_wave(A, bad)
    with pytest.raises(RuntimeError, match="sph_compute_matrices"):
        sph_zonal_averager(lat, lat_out, 4, lon=lon, wave_form="classes", device=99).sph_wave(A, 1)
