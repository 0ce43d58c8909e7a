"""Time-mean TEM, host side: the ctypes table against include/temx_clim.h and the plain-C link check, the launch shapes
of the time sum (pytemdiags_amd/csrc/clim_shapes.hpp, which needs no HIP) run on their own under AddressSanitizer +
UBSan, the front end's refusals before any device call, and the construction of the stationary / transient split in
numpy only.  Needs no GPU.

Bounds of the numpy construction (ne4 x 6 levels, L = 20, mode="factorised"): transient = total - stationary equals the
time mean of the zonal-mean products of the deviations from the time mean to 1e-10 of the total's maximum (observed
<= 2.2e-12: the identity is exact, the difference is the rounding of two fp64 pipelines), and stationary + transient =
total for the four results that are linear and homogeneous in the fluxes to 1e-12 (observed 3e-15)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import tem_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
ZM7 = ("ub", "vb", "thetab", "wapb", "upvpb", "upwappb", "vptpb")
FLUXES = ZM7[4:]
LINEAR = ("epfy", "epfz", "epdiv", "utendepfd")
_refs = {}


# ---- the reference of a climatology, in numpy (shared with tests/test_gpu_clim.py) ---------------------------------
def clim_reference(fields, lat, plev, L, key=None):
    """-> dict: ``full`` the per-snapshot oracle, ``stat`` the oracle of the time-mean fields, ``zm`` the seven zonal
    means of each set ({"total" | "stationary" | "transient": {name: (M, nlev, 1)}}), ``sets`` the epilogue oracle of
    each.  Computed once per ``key``, shared, left unchanged."""
    if key is not None and key in _refs:
        return _refs[key]
    f = [np.asarray(x, dtype=np.float64) for x in fields]
    full = orc.TEMOracle(*f, lat, plev, L=L, mode="factorised")
    stat = orc.TEMOracle(*[x.mean(axis=2, keepdims=True) for x in f], lat, plev, L=L, mode="factorised")
    tm = {n: getattr(full, n).mean(axis=2, keepdims=True) for n in ZM7}
    zm = {"total": dict(tm), "stationary": dict(tm), "transient": dict(tm)}
    for n in FLUXES:
        zm["stationary"][n] = getattr(stat, n)
        zm["transient"][n] = tm[n] - getattr(stat, n)
    ref = {"full": full, "stat": stat, "zm": zm,
           "sets": {k: orc.TEMOracle.from_zonal_means(v, full.plev) for k, v in zm.items()}}
    if key is not None:
        _refs[key] = ref
    return ref


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_clim_header_declares_exactly_what_is_bound():
    import ctypes as C
    from pytemdiags_amd import _clim, _lib
    hdr = open(os.path.join(ROOT, "include", "temx_clim.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(temxc_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _clim.SIGNATURES} == {"temxc_version", "temxc_time_sum",
                                                               "temxc_tem_from_zonal_means"}
    assert not re.findall(r"\b(temx[vli]?_[a-z0-9_]+)\s*\(", code)      # the other headers' ABI is not extended from here
    lib = _clim.load()
    assert lib is _lib.load() and lib.temxc_version() == _clim.CLIM_VERSION == 100
    for name, value in (("TEMXC_NF_MAX", _clim.NF_MAX), ("TEMXC_ACCUMULATE", _clim.ACCUMULATE)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "double*": C.c_void_p, "temx_plan*": C.c_void_p,
             "const void* const*": C.POINTER(C.c_void_p), "double* const*": C.POINTER(C.c_void_p),
             "const int*": C.POINTER(C.c_int)}
    sig = dict((n, (r, a)) for n, r, a in _clim.SIGNATURES)
    names = {}
    for fn in ("temxc_time_sum", "temxc_tem_from_zonal_means"):
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert sig[fn] == (C.c_int, [ctype[p.rsplit(" ", 1)[0]] for p in params]), fn
        names[fn] = [p.rsplit(" ", 1)[1] for p in params]
    assert sig["temxc_version"] == (C.c_int, [])
    assert names["temxc_time_sum"] == ["device", "nf", "src_host", "src_dtype_host", "acc_host", "ncol", "nlev", "nt",
                                       "flags", "stream"]
    assert names["temxc_tem_from_zonal_means"] == ["plan", "zm8", "nts", "results", "zonal_or_null", "stream"]
    # the entry points with a body are function-try-blocks, like every other one; the other versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    for fn in ("temxc_time_sum", "temxc_tem_from_zonal_means"):
        assert re.search(r"^int %s\([^;{]*\)\s*try \{\s*$" % fn, src, re.M), fn
    assert "int temx_version(void) { return 402; }" in src and "int temxl_version(void) { return 100; }" in src
    # the first header is as it was: nothing of this feature is declared there
    assert "temxc_" not in open(os.path.join(ROOT, "include", "temx.h")).read()


def test_clim_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_clim")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_clim.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxc_version=100 nf0_rc=-1 null_plan_rc=-1" in out.stdout
    assert "temx_version=402" in out.stdout


def test_time_sum_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _clim
    lib = _clim.load()
    src, acc = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(1 << 20)
    f64 = (C.c_int * 1)(0)

    def call(nf=1, src=src, sdt=f64, acc=acc, ncol=4, nlev=3, nt=5, flags=0):
        # device 99 does not exist: a call that got as far as the device would come back TEMX_EHIP, not TEMX_EINVAL
        return lib.temxc_time_sum(99, nf, src, sdt, acc, ncol, nlev, nt, flags, None)
    assert call(nf=0) == -1 and b"nf" in lib.temx_last_error()
    assert call(nf=9) == -1
    assert call(src=None) == -1 and call(acc=None) == -1 and call(sdt=None) == -1
    assert call(src=(C.c_void_p * 1)(None)) == -1 and call(acc=(C.c_void_p * 1)(None)) == -1
    assert call(sdt=(C.c_int * 1)(2)) == -1 and b"dtype" in lib.temx_last_error()
    assert call(flags=2) == -1 and b"flags" in lib.temx_last_error()
    assert call(ncol=0) == -1 and call(nlev=0) == -1 and call(nt=0) == -1
    assert call(src=(C.c_void_p * 1)(4100)) == -1 and b"aligned" in lib.temx_last_error()      # fp64 at 4 mod 8
    assert call(acc=(C.c_void_p * 1)((1 << 20) + 4)) == -1 and b"aligned" in lib.temx_last_error()
    assert call(src=(C.c_void_p * 1)(4100), sdt=(C.c_int * 1)(1)) == -2                          # fp32 at 4 mod 8 is aligned
    # src is 4 * 3 * 5 * 8 = 480 bytes at 4096, acc 96 bytes
    assert call(acc=(C.c_void_p * 1)(4096 + 472)) == -1 and b"overlaps src" in lib.temx_last_error()
    assert call(acc=(C.c_void_p * 1)(4096 - 88)) == -1 and b"overlaps src" in lib.temx_last_error()
    assert call(acc=(C.c_void_p * 1)(4096 + 480)) == -2 and call(acc=(C.c_void_p * 1)(4096 - 96)) == -2   # touching is fine
    two = dict(nf=2, src=(C.c_void_p * 2)(4096, 8192), sdt=(C.c_int * 2)(0, 1))
    assert call(acc=(C.c_void_p * 2)(1 << 20, (1 << 20) + 88), **two) == -1 and b"overlaps acc" in lib.temx_last_error()
    assert call(acc=(C.c_void_p * 2)(1 << 20, (1 << 20) + 96), **two) == -2
    assert call() == -2 and call(flags=_clim.ACCUMULATE) == -2       # well-formed: only now is the device touched
    assert lib.temxc_tem_from_zonal_means(None, C.c_void_p(4096), 1, C.c_void_p(8192), None, None) == -1


# ---- clim_shapes.hpp on its own, under the sanitizers ------------------------------------------------------------------
def test_clim_shapes_rows_owned_once_lds_budget_and_switch_point(tmp_path):
    """tests/host/clim_shapes_main.cpp walks every launch shape for nt = 1..2000, both dtypes and a few row counts: every
    row owned exactly once, the staged bytes inside the LDS budget, the kernel switching exactly at clim_switch_nt."""
    from pytemdiags_amd import _clim
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")
    exe = str(tmp_path / "clim_shapes_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                    os.path.join(ROOT, "tests", "host", "clim_shapes_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"switch_f64=(\d+) switch_f32=(\d+) cases=(\d+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) == _clim.switch_nt(8) and int(m.group(2)) == _clim.switch_nt(4)
    assert int(m.group(3)) == 2 * 2000 * 8
    # the two long records of the issue straddle it: ne30 x 72 x 92 is staged, ne30 x 72 x 730 takes the long rows
    assert 92 < _clim.switch_nt(8) <= 730 and 92 < _clim.switch_nt(4) <= 730
    # the constants the Python mirror is computed from are the header's
    hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "clim_shapes.hpp")).read()
    assert re.search(r"CLIM_THREADS = %d;" % _clim.THREADS, hpp)
    assert re.search(r"CLIM_LDS_BYTES = %d \* 1024;" % (_clim.LDS_BYTES // 1024), hpp)
    assert re.search(r"CLIM_MIN_ROWS = %d;" % _clim.MIN_ROWS, hpp)
    assert re.search(r"CLIM_NFMAX = %d;" % _clim.NF_MAX, hpp)


# ---- front-end refusals before the device -------------------------------------------------------------------------------
def _tiny():
    la = -90 + (np.arange(6) + 0.5) * 30.0
    lat = np.repeat(la, 8)
    plev = np.array([100.0, 500.0, 1000.0])
    f = np.zeros((lat.size, 3, 2))
    return lat, plev, f


def test_climatology_with_mask_is_refused_before_device():
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match="climatology"):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, climatology=True, missing="mask", device=99)
    with pytest.raises(ValueError, match="climatology"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=plev, ps=np.zeros((lat.size, 2)), hyam=np.zeros(3),
                                         hybm=np.ones(3), climatology=True, missing="mask", device=99)


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0, (True,)])
def test_climatology_must_be_a_bool_before_device(bad):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match="climatology"):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, climatology=bad, device=99)


def test_climatology_is_keyword_only_and_off_by_default():
    import inspect
    from pytemdiags_amd import TEMDiagnostics, climatology
    p = inspect.signature(TEMDiagnostics.__init__).parameters["climatology"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert isinstance(TEMDiagnostics.climatology, property)
    assert set(climatology.TIME_SUM_KERNEL) == {"float64", "float32"}
    assert all(isinstance(v, bool) for v in climatology.TIME_SUM_KERNEL.values())
    # the result sets offer the names of TEMDiagnostics
    from pytemdiags_amd import _lib
    for n in _lib.RESULT_NAMES:
        assert callable(getattr(climatology.ResultSet, n)) and callable(getattr(TEMDiagnostics, n))
    for n in _lib.ZONAL_NAMES:
        assert isinstance(getattr(climatology.ResultSet, n), property) and isinstance(getattr(TEMDiagnostics, n), property)


def test_time_sum_gate_is_backed_by_a_committed_measurement():
    """``climatology.TIME_SUM_KERNEL`` switches the kernel on for a dtype exactly where profiles/clim_bench_mi355x.json
    shows it faster than torch.sum at ne120 x 72 x 30."""
    import json
    from pytemdiags_amd import climatology
    path = os.path.join(ROOT, "profiles", "clim_bench_mi355x.json")
    assert os.path.exists(path), "TIME_SUM_KERNEL without a measurement"
    legs = json.load(open(path))["time_sum"]
    for name, on in climatology.TIME_SUM_KERNEL.items():
        leg = [r for r in legs if (r["ncol"], r["nlev"], r["nt"], r["dtype"]) == (777602, 72, 30, name)]
        assert len(leg) == 1, name
        assert on == (leg[0]["torch_over_kernel_time"] > 1.0), (name, leg[0])


def test_mean_time_of_numbers_and_dates():
    from pytemdiags_amd.climatology import mean_time
    np.testing.assert_array_equal(mean_time(np.arange(5)), [2.0])
    np.testing.assert_array_equal(mean_time(np.zeros(1)), [0.0])
    d = np.array(["2001-01-01", "2001-01-03", "2001-01-08"], dtype="datetime64[D]")
    assert mean_time(d)[0] == np.datetime64("2001-01-04") and mean_time(d).shape == (1,)


# ---- the construction, in numpy only -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [3, 6])
def test_transient_is_total_minus_stationary_and_linear_results_add_up(nt):
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(4)[:2]
    plev = synth.pressure_levels(6)
    f = synth.analytic_fields(lat, lon, plev, nt, seed=3)
    ref = clim_reference(f, lat, plev, 20)
    full, stat, zm = ref["full"], ref["stat"], ref["zm"]
    # the mean state of the two routes agrees: the operator is linear and does not depend on time
    for n in ZM7[:4]:
        assert np.abs(getattr(stat, n) - zm["total"][n]).max() <= 1e-12 * np.abs(zm["total"][n]).max(), n
    # the transient fluxes, directly: zonal means of the products of the deviations from the time mean, time-averaged
    dev = {n: getattr(full, n) - getattr(stat, n) for n in ("up", "vp", "thetap", "wapp")}
    direct = {"upvpb": dev["up"] * dev["vp"], "upwappb": dev["up"] * dev["wapp"], "vptpb": dev["vp"] * dev["thetap"]}
    for n in FLUXES:
        d = full.ZM.zonal_mean(direct[n]).mean(axis=2, keepdims=True)
        top = np.abs(zm["total"][n]).max()
        e = np.abs(zm["transient"][n] - d).max() / top
        share = np.abs(zm["transient"][n]).max() / top
        print("nt=%d %s: transient vs direct %.2e of the total's maximum, transient share %.3f" % (nt, n, e, share))
        assert e <= 1e-10, (n, e)
        assert share > 1e-3, (n, share)              # there is a transient part to speak of
    # stationary + transient = total for the four results that are linear and homogeneous in the fluxes
    S, T, tot = (ref["sets"][k] for k in ("stationary", "transient", "total"))
    for n in LINEAR:
        e = np.abs(getattr(S, n)() + getattr(T, n)() - getattr(tot, n)()).max() / np.abs(getattr(tot, n)()).max()
        print("nt=%d %s: S + T - total %.2e" % (nt, n, e))
        assert e <= 1e-12, (n, e)
    # ... and not for the others: they carry the mean-state term in every set
    assert np.abs(S.vtem() + T.vtem() - tot.vtem()).max() > 1e-3 * np.abs(tot.vtem()).max()
