"""Time-mean TEM of fields with missing values (masked climatology), host side: the ctypes table against
include/temx_nclim.h and the plain-C link check, the argument checks of temxn_time_sum_valid before any device call,
the launch shapes (pytemdiags_amd/csrc/nclim_shapes.hpp, which needs no HIP) run on their own under AddressSanitizer +
UBSan, the front end's refusals before any device call, and the numpy reference of the masked climatology with its
self-checks.  Needs no GPU.

Bounds of the reference's self-checks: on NaN-free input the masked reference equals ``test_clim_host.clim_reference``
to 1e-12 of each quantity's maximum (the masked oracle's lstsq against the default pipeline, on the 24 x 16 lat-lon
grid at L = 12 where tests/test_missing_host.py holds the two to that bound), and stationary + transient = total for the four results that are
linear and homogeneous in the fluxes to 1e-12 where all three are finite."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import tem_oracle as orc
from test_clim_host import FLUXES, LINEAR, ZM7, clim_reference
from test_missing_host import MaskedOracle, surface_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SETS = ("total", "stationary", "transient")
_refs = {}


# ---- the reference of a masked climatology, in numpy (shared with tests/test_gpu_nclim.py) ---------------------------
def times_needed(v, nt):
    return max(1, int(math.ceil(v * nt - 1e-9)))


def counted_mean(x, valid, need):
    """Sum over the valid entries of the last axis over their count, NaN where the count is below ``need``
    -> (mean with a last axis of 1, count)."""
    cnt = valid.sum(axis=-1)
    s = np.sum(np.where(valid, x, 0.0), axis=-1)
    with np.errstate(all="ignore"):
        m = np.where(cnt >= need, s / cnt, np.nan)
    return m[..., None], cnt


def masked_clim_reference(fields, lat, plev, L, min_coverage, min_time_coverage, key=None):
    """-> dict: ``full`` the per-snapshot MaskedOracle, ``means`` the four counted and thresholded time-mean fields
    (ncol, nlev, 1) with ``count`` their common count, ``stat`` the MaskedOracle of those, ``time_coverage`` (M, nlev, 1),
    ``zcount`` the count of finite snapshots on the zonal grid, ``zm`` the seven zonal means of each set and ``sets``
    the epilogue oracle of each.  Computed once per ``key``, shared, left unchanged."""
    if key is not None and key in _refs:
        return _refs[key]
    f = [np.asarray(x, dtype=np.float64) for x in fields]
    N, nlev, nt = f[0].shape
    need = times_needed(min_time_coverage, nt)
    full = MaskedOracle(*f, lat, plev, L, min_coverage=min_coverage)
    valid = ~full.miss.reshape(N, nlev, nt)                                  # the common mask of the four
    means, count = [], None
    for x in f:
        m, count = counted_mean(x, valid, need)
        means.append(m)
    stat = MaskedOracle(*means, lat, plev, L, min_coverage=min_coverage)
    tm, zcount = {}, None
    for n in ZM7:
        z = full.zonal[n]
        tm[n], c = counted_mean(z, np.isfinite(z), need)
        assert zcount is None or np.array_equal(c, zcount), n               # the seven share their NaN pattern
        zcount = c
    zm = {"total": dict(tm), "stationary": dict(tm), "transient": dict(tm)}
    for n in FLUXES:
        zm["stationary"][n] = stat.zonal[n]
        zm["transient"][n] = tm[n] - stat.zonal[n]
    with np.errstate(all="ignore"):
        sets = {k: orc.TEMOracle.from_zonal_means(v, full.plev) for k, v in zm.items()}
        values = {k: dict(o.results(), **o.zonal_attrs()) for k, o in sets.items()}
    ref = {"full": full, "means": means, "count": count, "stat": stat, "need": need, "zcount": zcount,
           "time_coverage": (zcount / float(nt))[..., None], "zm": zm, "sets": sets, "values": values}
    if key is not None:
        _refs[key] = ref
    return ref


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_nclim_header_declares_exactly_what_is_bound():
    import ctypes as C
    from pytemdiags_amd import _nclim, _lib
    hdr = open(os.path.join(ROOT, "include", "temx_nclim.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(temxn_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _nclim.SIGNATURES} == {"temxn_version", "temxn_time_sum_valid"}
    assert not re.findall(r"\b(temx[vlicm]?_[a-z0-9_]+)\s*\(", code)     # no other prefix is declared here
    lib = _nclim.load()
    assert lib is _lib.load() and lib.temxn_version() == _nclim.NCLIM_VERSION == 100
    for name, value in (("TEMXN_NF_MAX", _nclim.NF_MAX), ("TEMXN_ACCUMULATE", _nclim.ACCUMULATE),
                        ("TEMXN_COMMON_MASK", _nclim.COMMON_MASK)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    assert (_nclim.NF_MAX, _nclim.ACCUMULATE, _nclim.COMMON_MASK) == (8, 1, 2)
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const void* const*": C.POINTER(C.c_void_p),
             "double* const*": C.POINTER(C.c_void_p)}
    sig = dict((n, (r, a)) for n, r, a in _nclim.SIGNATURES)
    decl = re.search(r"int temxn_time_sum_valid\((.*?)\);", code, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert sig["temxn_time_sum_valid"] == (C.c_int, [ctype[p.rsplit(" ", 1)[0]] for p in params])
    assert [p.rsplit(" ", 1)[1] for p in params] == ["device", "nf", "src_host", "src_dtype", "acc_host", "cnt_host", "ncol",
                                                     "nlev", "nt", "flags", "stream"]
    assert sig["temxn_version"] == (C.c_int, [])
    # the entry point is a function-try-block, like every other one; the other versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    assert re.search(r"^int temxn_time_sum_valid\([^;{]*\)\s*try \{\s*$", src, re.M)
    assert "int temx_version(void) { return 402; }" in src and "int temxn_version(void) { return 100; }" in src
    for fn in ("temxv", "temxl", "temxi", "temxc", "temxm"):
        assert "int %s_version(void) { return 100; }" % fn in src, fn
    # the other six headers are as they were: nothing of this feature is declared there
    for h in ("temx.h", "temx_vert.h", "temx_layout.h", "temx_ingest.h", "temx_clim.h", "temx_mtracer.h"):
        assert "temxn_" not in open(os.path.join(ROOT, "include", h)).read(), h
    from pytemdiags_amd import _clim, _ingest, _layout, _mtracer, _vert
    assert (_lib.ABI_VERSION, _vert.VERT_VERSION, _layout.LAYOUT_VERSION, _ingest.INGEST_VERSION, _clim.CLIM_VERSION,
            _mtracer.MTRACER_VERSION) == (402, 100, 100, 100, 100, 100)


def test_nclim_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_nclim")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_nclim.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxn_version=100 nf0_rc=-1" in out.stdout
    assert "temx_version=402" in out.stdout


def test_time_sum_valid_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _nclim
    lib = _nclim.load()
    P = C.c_void_p
    src, acc, cnt = (P * 1)(4096), (P * 1)(1 << 20), (P * 1)(1 << 21)

    def call(nf=1, src=src, dt=0, acc=acc, cnt=cnt, ncol=4, nlev=3, nt=5, flags=0):
        # device 99 does not exist: a call that got as far as the device would come back TEMX_EHIP, not TEMX_EINVAL
        return lib.temxn_time_sum_valid(99, nf, src, dt, acc, cnt, ncol, nlev, nt, flags, None)

    def err():
        return lib.temx_last_error()
    assert call(nf=0) == -1 and b"nf" in err()
    assert call(nf=9) == -1 and b"nf" in err()
    assert call(src=None) == -1 and b"src_host" in err()
    assert call(acc=None) == -1 and b"acc_host" in err()
    assert call(cnt=None) == -1 and b"cnt_host" in err()
    assert call(src=(P * 1)(None)) == -1 and b"src 0 is null" in err()
    assert call(acc=(P * 1)(None)) == -1 and b"acc 0 is null" in err()
    assert call(cnt=(P * 1)(None)) == -1 and b"cnt 0 is null" in err()
    assert call(dt=2) == -1 and b"dtype" in err()
    assert call(dt=-1) == -1 and b"dtype" in err()
    assert call(flags=4) == -1 and b"flags" in err()
    assert call(flags=8 | 1) == -1 and b"flags" in err()
    assert call(ncol=0) == -1 and b"ncol" in err()
    assert call(nlev=0) == -1 and b"nlev" in err()
    assert call(nt=0) == -1 and b"nt" in err()
    assert call(src=(P * 1)(4100)) == -1 and b"src 0 is not aligned" in err()           # fp64 at 4 mod 8
    assert call(acc=(P * 1)((1 << 20) + 4)) == -1 and b"acc 0 is not aligned" in err()
    assert call(cnt=(P * 1)((1 << 21) + 4)) == -1 and b"cnt 0 is not aligned" in err()
    assert call(src=(P * 1)(4100), dt=1) == -2                                          # fp32 at 4 mod 8 is aligned
    assert call(src=(P * 1)(4098), dt=1) == -1 and b"aligned" in err()
    # src is 4 * 3 * 5 * 8 = 480 bytes at 4096, acc and cnt 96 bytes each
    assert call(acc=(P * 1)(4096 + 472)) == -1 and b"acc 0 overlaps src 0" in err()
    assert call(acc=(P * 1)(4096 - 88)) == -1 and b"acc 0 overlaps src 0" in err()
    assert call(cnt=(P * 1)(4096 + 472)) == -1 and b"cnt 0 overlaps src 0" in err()
    assert call(cnt=(P * 1)(4096 - 88)) == -1 and b"cnt 0 overlaps src 0" in err()
    assert call(cnt=(P * 1)((1 << 20) + 88)) == -1 and b"cnt 0 overlaps acc 0" in err()
    assert call(cnt=(P * 1)((1 << 20) - 88)) == -1 and b"cnt 0 overlaps acc 0" in err()
    assert call(acc=(P * 1)(4096 + 480)) == -2 and call(cnt=(P * 1)(4096 - 96)) == -2      # touching is fine
    assert call(cnt=(P * 1)((1 << 20) + 96)) == -2
    two = dict(nf=2, src=(P * 2)(4096, 8192))
    a2, c2 = (P * 2)(1 << 20, (1 << 20) + 96), (P * 2)(1 << 21, (1 << 21) + 96)
    assert call(acc=(P * 2)(1 << 20, (1 << 20) + 88), cnt=c2, **two) == -1 and b"acc 1 overlaps acc 0" in err()
    assert call(acc=a2, cnt=(P * 2)(1 << 21, (1 << 21) + 88), **two) == -1 and b"cnt 1 overlaps cnt 0" in err()
    assert call(acc=a2, cnt=(P * 2)(1 << 21, (1 << 20) + 100), **two) == -1                # the second count on acc 1
    assert call(acc=a2, cnt=(P * 2)(1 << 21, 8192 + 8), **two) == -1 and b"cnt 1 overlaps src 1" in err()
    assert call(acc=a2, cnt=(P * 2)(1 << 21, None), **two) == -1 and b"cnt 1 is null" in err()
    # under a common mask only cnt_host[0] is used: a null, misaligned or overlapping cnt_host[1] is not looked at
    for flags in (_nclim.COMMON_MASK, _nclim.COMMON_MASK | _nclim.ACCUMULATE):
        assert call(acc=a2, cnt=(P * 2)(1 << 21, None), flags=flags, **two) == -2
        assert call(acc=a2, cnt=(P * 2)(1 << 21, (1 << 20) + 4), flags=flags, **two) == -2
        assert call(acc=a2, cnt=(P * 2)(None, 1 << 21), flags=flags, **two) == -1 and b"cnt 0 is null" in err()
    assert call(acc=a2, cnt=c2, **two) == -2
    assert call() == -2 and call(flags=_nclim.ACCUMULATE) == -2      # well-formed: only now is the device touched
    assert call(flags=_nclim.COMMON_MASK) == -2 and call(dt=1) == -2


# ---- nclim_shapes.hpp on its own, under the sanitizers ---------------------------------------------------------------
def test_nclim_shapes_rows_owned_once_lds_budget_and_switch_point(tmp_path):
    """tests/host/nclim_shapes_main.cpp walks every launch shape for nt = 1..2000, both dtypes, nf = 1..8, both modes and
    a few row counts: every row owned exactly once, the staged bytes of all the fields a workgroup holds inside the LDS
    budget, the kernel switching exactly at the mirror's switch point."""
    from pytemdiags_amd import _nclim
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")
    exe = str(tmp_path / "nclim_shapes_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                    os.path.join(ROOT, "tests", "host", "nclim_shapes_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    sw = {(int(e), int(n)): int(nt) for e, n, nt in re.findall(r"switch esz=(\d+) nfs=(\d+) nt=(\d+)", out.stdout)}
    assert set(sw) == {(e, n) for e in (8, 4) for n in range(1, 9)}
    for (e, n), nt in sw.items():
        assert nt == _nclim.switch_nt(e, n, common=True), (e, n)
        assert _nclim.switch_nt(e, n, common=False) == sw[(e, 1)] == _nclim.switch_nt(e)   # own mask: a field per workgroup
        # the mirror's shape at both sides of the switch
        assert _nclim.shape(1000, nt - 1, e, n)["staged"] == 1 and _nclim.shape(1000, nt, e, n)["staged"] == 0
    m = re.search(r"cases=(\d+)", out.stdout)
    assert m and int(m.group(1)) == 2 * 2 * 8 * 2000 * 4
    # four fields at ne120 x 72 x 30 are staged in both dtypes; ne30 x 72 x 730 takes the long rows
    assert 30 < _nclim.switch_nt(8, 4, True) <= 730 and 30 < _nclim.switch_nt(4, 4, True) <= 730
    s = _nclim.shape(777602 * 72, 30, 8, 4)
    assert s["staged"] == 1 and 4 * s["rpb"] * s["stride"] * 8 <= _nclim.LDS_BYTES and s["rpb"] * s["g"] <= _nclim.THREADS
    # the constants the Python mirror is computed from are the header's
    hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "nclim_shapes.hpp")).read()
    assert re.search(r"NCLIM_THREADS = %d;" % _nclim.THREADS, hpp)
    assert re.search(r"NCLIM_LDS_BYTES = %d \* 1024;" % (_nclim.LDS_BYTES // 1024), hpp)
    assert re.search(r"NCLIM_MIN_ROWS = %d;" % _nclim.MIN_ROWS, hpp)
    assert re.search(r"NCLIM_NFMAX = %d;" % _nclim.NF_MAX, hpp)
    assert not re.search(r"#include\s*<hip", hpp)
    # five workgroups of that budget share a CU's 160 KiB
    assert 5 * _nclim.LDS_BYTES <= 160 * 1024


# ---- front-end refusals before the device ----------------------------------------------------------------------------
def _tiny():
    la = -90 + (np.arange(6) + 0.5) * 30.0
    lat = np.repeat(la, 8)
    plev = np.array([100.0, 500.0, 1000.0])
    f = np.zeros((lat.size, 3, 2))
    return lat, plev, f


def test_min_time_coverage_refusals_come_before_the_device():
    from pytemdiags_amd import TEMDiagnostics, climatology
    lat, plev, f = _tiny()

    def direct(**kw):
        return TEMDiagnostics(f, f, f, f, lat, plev=plev, device=99, **kw)

    def levels(**kw):
        return TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=plev, ps=np.zeros((lat.size, 2)), hyam=np.zeros(3),
                                                hybm=np.ones(3), device=99, **kw)
    for build in (direct, levels):
        with pytest.raises(ValueError, match="a contract of its own"):      # the old refusal stands without the keyword
            build(climatology=True, missing="mask")
        for bad in (0, 0.0, -0.5, 1.0000001, 2, "half", float("nan"), True, (0.5,)):
            with pytest.raises(ValueError, match="min_time_coverage"):
                build(climatology=True, missing="mask", min_time_coverage=bad)
        with pytest.raises(ValueError, match="min_time_coverage"):         # without missing="mask"
            build(climatology=True, min_time_coverage=0.5)
        with pytest.raises(ValueError, match="min_time_coverage"):         # without climatology=True
            build(missing="mask", min_time_coverage=0.5)
        with pytest.raises(ValueError, match="min_time_coverage"):
            build(min_time_coverage=0.5)
    # a good value gets past the checks: what stops the run now is the device that does not exist
    for v in (0.5, 1, 1.0, 1e-6, np.float32(0.25)):
        with pytest.raises(Exception) as ei:
            direct(climatology=True, missing="mask", min_time_coverage=v)
        assert not isinstance(ei.value, ValueError) or "min_time_coverage" not in str(ei.value), v
    # check_flag stays callable with two arguments
    assert climatology.check_flag(True, "raise") is True and climatology.check_flag(False, "mask") is False
    with pytest.raises(ValueError, match="climatology"):
        climatology.check_flag(True, "mask")
    assert climatology.check_flag(True, "mask", 0.5) is True
    assert [climatology.times_needed(0.5, n) for n in (1, 2, 5, 6)] == [1, 1, 3, 3]
    assert climatology.times_needed(1.0, 5) == 5 and climatology.times_needed(1e-6, 5) == 1
    assert climatology.times_needed(0.6, 5) == 3 == times_needed(0.6, 5)               # 0.6 * 5 = 3.0000000000000004


def test_min_time_coverage_is_keyword_only_and_off_by_default():
    import inspect
    from pytemdiags_amd import TEMDiagnostics, climatology
    p = inspect.signature(TEMDiagnostics.__init__).parameters["min_time_coverage"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert issubclass(climatology.MaskedBuilder, climatology.Builder)
    assert isinstance(climatology.TEMClimatology.time_coverage, property)
    assert isinstance(climatology.TEMClimatology.stationary_coverage, property)


# ---- the numpy reference: self-checks --------------------------------------------------------------------------------
def _fields(nt, seed=3, nlev=6):
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(4)[:2]
    plev = synth.pressure_levels(nlev)
    return lat, lon, plev, synth.analytic_fields(lat, lon, plev, nt, seed=seed)


def test_masked_reference_on_nan_free_input_is_the_unmasked_reference():
    """On the grid and degree at which the masked oracle's lstsq is known to agree with the default pipeline to 1e-12
    (test_missing_host.test_masked_oracle_without_missing_points_is_the_default_pipeline: 24 x 16 lat-lon, L = 12)."""
    from pytemdiags_amd import synth
    from test_missing_host import latlon
    lat, lon = latlon(24, 16)
    plev = synth.pressure_levels(8)
    f = synth.analytic_fields(lat, lon, plev, 3, seed=5)
    ref = masked_clim_reference(f, lat, plev, 12, 0.5, 0.5)
    plain = clim_reference(f, lat, plev, 12)
    assert np.all(ref["time_coverage"] == 1.0) and np.all(ref["count"] == 3) and ref["need"] == 2
    want = {"total": plain["sets"]["total"], "stationary": plain["stat"], "transient": plain["sets"]["transient"]}
    worst = (0.0, "")
    for s in SETS:
        w = dict(want[s].results(), **want[s].zonal_attrs())
        for n, r in w.items():
            e = float(np.max(np.abs(ref["values"][s][n] - r)) / max(np.max(np.abs(r)), 1e-300))
            worst = max(worst, (e, "%s.%s" % (s, n)))
            assert e <= 1e-12, (s, n, e)
    print("masked reference against the unmasked one, NaN-free input: worst %.2e (%s)" % worst)


def test_masked_reference_linear_results_add_up_where_finite():
    lat, lon, plev, f = _fields(5, seed=1, nlev=8)
    plev = np.sort(plev * 0.5 + 500.0 * np.linspace(0, 1, 8) ** 2)
    miss = surface_mask(lat, lon, plev, 5)
    f = [np.where(miss, np.nan, x) for x in f]
    ref = masked_clim_reference(f, lat, plev, 20, 0.5, 0.5)
    v = ref["values"]
    some = 0
    for n in LINEAR:
        fin = np.isfinite(v["total"][n]) & np.isfinite(v["stationary"][n]) & np.isfinite(v["transient"][n])
        assert fin.any() and not fin.all(), n
        e = np.abs(v["stationary"][n] + v["transient"][n] - v["total"][n])[fin].max() / np.abs(v["total"][n][fin]).max()
        print("%s: S + T - total %.2e on %d finite points" % (n, e, fin.sum()))
        assert e <= 1e-12, (n, e)
        some += int(fin.sum())
    assert some
    # the mean fields are missing where the count is below need, and nowhere else
    assert np.array_equal(np.isnan(ref["means"][0][..., 0]), ref["count"] < ref["need"])
    assert (ref["count"] == 0).any() and ((ref["count"] > 0) & (ref["count"] < 5)).any()
