"""Grouped and weighted time means, host side: the ctypes table against include/temx_gclim.h and the plain-C link check,
the argument checks of temxg_time_sum_groups before any device call, the tables of the grouped sum
(pytemdiags_amd/csrc/gclim_tables.hpp, which needs no HIP) on their own under AddressSanitizer + UBSan, the front end's
refusals before any device call, ``climatology.calendar_groups``, and the construction of the grouped stationary /
transient split in numpy only.  Needs no GPU.

Bounds of the numpy construction (ne4 x 6 levels x 7 times, L = 20, mode="factorised", labels [1,0,-1,1,0,1,1], weights
[1,.5,3,2,.25,1,0]), those of tests/test_clim_host.py: the group-mean state by the two routes (zonal means of the group
means, group means of the zonal means) to 1e-12 (observed 3e-15), a transient share above 1e-3 in every group (observed
0.11 .. 0.58), the stationary run of both groups at once against one run per group to 1e-12 (observed 6e-15), and
stationary + transient = total for the four flux-linear results per group to 1e-12."""
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
LABELS = np.array([1, 0, -1, 1, 0, 1, 1])
WEIGHTS = np.array([1, .5, 3, 2, .25, 1, 0])
_refs = {}


# ---- the reference of a grouped climatology, in numpy (shared with tests/test_gpu_gclim.py) -------------------------
def weight_matrix(labels, weights, nt):
    """``Wm[t][g] = w_t [label_t == g]`` and the total weight of each group."""
    labels = np.asarray(labels)
    w = np.ones(nt) if weights is None else np.asarray(weights, dtype=np.float64)
    ng = int(labels.max()) + 1
    wm = np.zeros((nt, ng))
    keep = np.nonzero(labels >= 0)[0]
    wm[keep, labels[keep]] = w[keep]
    return wm, wm.sum(axis=0)


def group_mean(x, wm, wsum):
    """Weighted group means over the last axis, ``(..., nt) -> (..., G)``.  Times that carry no weight in any group are
    cut out first: a left-out time never enters, whatever it holds (in a matrix product 0 * NaN would)."""
    used = np.nonzero(wm.any(axis=1))[0]
    return np.tensordot(np.asarray(x, dtype=np.float64)[..., used], wm[used], axes=([-1], [0])) / wsum


def gclim_reference(fields, lat, plev, L, labels, weights, key=None):
    """-> dict: ``full`` the per-snapshot oracle, ``stat`` the oracle of the group-mean fields (G snapshots), ``zm`` the
    seven zonal means of each set ({"total" | "stationary" | "transient": {name: (M, nlev, G)}}), ``sets`` the epilogue
    oracle of each, ``wm`` / ``wsum`` the weight matrix and the groups' total weights.  Computed once per ``key``,
    shared, left unchanged."""
    if key is not None and key in _refs:
        return _refs[key]
    f = [np.asarray(x, dtype=np.float64) for x in fields]
    wm, wsum = weight_matrix(labels, weights, f[0].shape[2])
    full = orc.TEMOracle(*f, lat, plev, L=L, mode="factorised")
    stat = orc.TEMOracle(*[group_mean(x, wm, wsum) for x in f], lat, plev, L=L, mode="factorised")
    tm = {n: group_mean(getattr(full, n), wm, wsum) for n in ZM7}
    zm = {"total": dict(tm), "stationary": dict(tm), "transient": dict(tm)}
    for n in FLUXES:
        zm["stationary"][n] = getattr(stat, n)
        zm["transient"][n] = tm[n] - getattr(stat, n)
    ref = {"full": full, "stat": stat, "zm": zm, "wm": wm, "wsum": wsum,
           "sets": {k: orc.TEMOracle.from_zonal_means(v, full.plev) for k, v in zm.items()}}
    if key is not None:
        _refs[key] = ref
    return ref


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_gclim_header_declares_exactly_what_is_bound():
    import ctypes as C
    from pytemdiags_amd import _gclim, _lib
    hdr = open(os.path.join(ROOT, "include", "temx_gclim.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(temxg_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _gclim.SIGNATURES} == {"temxg_version", "temxg_time_sum_groups"}
    assert not re.findall(r"\b(temx[vlicnm]?_[a-z0-9_]+)\s*\(", code)   # the other headers' ABI is not extended from here
    lib = _gclim.load()
    assert lib is _lib.load() and lib.temxg_version() == _gclim.GCLIM_VERSION == 100
    for name, value in (("TEMXG_NF_MAX", _gclim.NF_MAX), ("TEMXG_NG_MAX", _gclim.NG_MAX), ("TEMXG_ACCUMULATE", _gclim.ACCUMULATE)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const void* const*": C.POINTER(C.c_void_p),
             "double* const*": C.POINTER(C.c_void_p), "const int*": C.POINTER(C.c_int),
             "const int32_t*": C.POINTER(C.c_int32), "const double*": C.POINTER(C.c_double)}
    sig = dict((n, (r, a)) for n, r, a in _gclim.SIGNATURES)
    decl = re.search(r"int temxg_time_sum_groups\((.*?)\);", code, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert sig["temxg_time_sum_groups"] == (C.c_int, [ctype[p.rsplit(" ", 1)[0]] for p in params])
    assert sig["temxg_version"] == (C.c_int, [])
    assert [p.rsplit(" ", 1)[1] for p in params] == [
        "device", "nf", "src_host", "src_dtype_host", "acc_host", "ncol", "nlev", "nt", "nt_record", "t0", "ng", "label_host",
        "weight_host_or_null", "flags", "stream"]
    # the entry point is a function-try-block, like every other one; the other versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    assert re.search(r"^int temxg_time_sum_groups\([^;{]*\)\s*try \{\s*$", src, re.M)
    for fn, v in (("temx", 402), ("temxv", 100), ("temxl", 100), ("temxi", 100), ("temxc", 100), ("temxm", 100),
                  ("temxn", 100), ("temxg", 100)):
        assert "int %s_version(void) { return %d; }" % (fn, v) in src, fn
    # the other seven headers are as they were: nothing of this feature is declared there
    others = sorted(n for n in os.listdir(os.path.join(ROOT, "include")) if n != "temx_gclim.h")
    assert others == ["temx.h", "temx_clim.h", "temx_ingest.h", "temx_layout.h", "temx_mtracer.h", "temx_nclim.h", "temx_vert.h"]
    for n in others:
        assert "temxg_" not in open(os.path.join(ROOT, "include", n)).read(), n
    # the instantiations of the long-row kernel are those the bindings name
    hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "dispatch.hpp")).read()
    assert hpp.count("IntList<%s>" % ", ".join(str(b) for b in _gclim.BOUNDS)) == 1
    assert [_gclim.bound(n) for n in (1, 2, 4, 5, 16, 17, 64)] == [1, 4, 4, 64, 64, 64, 64]


def test_gclim_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_gclim")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_gclim.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxg_version=100 nf0_rc=-1 ng65_rc=-1" in out.stdout
    assert "temx_version=402" in out.stdout


def test_time_sum_groups_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _gclim
    lib = _gclim.load()
    src, acc = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(1 << 20)
    f64 = (C.c_int * 1)(0)
    lab5 = (C.c_int32 * 5)(0, 1, -1, 1, 0)
    w5 = (C.c_double * 5)(1.0, 0.5, 3.0, 2.0, 0.0)

    def call(nf=1, src=src, sdt=f64, acc=acc, ncol=4, nlev=3, nt=5, ntr=5, t0=0, ng=2, lab=lab5, w=w5, flags=0):
        # device 99 does not exist: a call that got as far as the device would come back TEMX_EHIP, not TEMX_EINVAL
        return lib.temxg_time_sum_groups(99, nf, src, sdt, acc, ncol, nlev, nt, ntr, t0, ng, lab, w, flags, None)
    err = lib.temx_last_error
    # every bad argument of the temxc_time_sum test
    assert call(nf=0) == -1 and b"nf" in err()
    assert call(nf=9) == -1
    assert call(src=None) == -1 and call(acc=None) == -1 and call(sdt=None) == -1
    assert call(src=(C.c_void_p * 1)(None)) == -1 and call(acc=(C.c_void_p * 1)(None)) == -1
    assert call(sdt=(C.c_int * 1)(2)) == -1 and b"dtype" in err()
    assert call(flags=2) == -1 and b"flags" in err()
    assert call(ncol=0) == -1 and call(nlev=0) == -1 and call(nt=0) == -1
    assert call(src=(C.c_void_p * 1)(4100)) == -1 and b"aligned" in err()      # fp64 at 4 mod 8
    assert call(acc=(C.c_void_p * 1)((1 << 20) + 4)) == -1 and b"aligned" in err()
    assert call(src=(C.c_void_p * 1)(4100), sdt=(C.c_int * 1)(1)) == -2         # fp32 at 4 mod 8 is aligned
    # the group arguments
    assert call(ng=0) == -1 and b"ng must lie in 1..64" in err()
    assert call(ng=65) == -1 and b"ng must lie in 1..64" in err()
    assert call(t0=-1, nt=2) == -1 and b"t0 must not be negative" in err()
    assert call(t0=1) == -1 and b"exceeds nt_record" in err()
    assert call(nt=6) == -1 and b"exceeds nt_record" in err()
    assert call(lab=None) == -1 and b"label_host" in err()
    assert call(lab=(C.c_int32 * 5)(0, 1, -2, 1, 0)) == -1 and b"label 2 is -2" in err()
    assert call(lab=(C.c_int32 * 5)(0, 1, -1, 2, 0)) == -1 and b"label 3 is 2" in err()
    assert call(ng=1) == -1 and b"label 1 is 1" in err()
    for v in (-0.5, float("nan"), float("inf")):
        assert call(w=(C.c_double * 5)(1.0, 0.5, v, 2.0, 0.0)) == -1 and b"weight 2 must be finite and not negative" in err()
    # src is 4 * 3 * 5 * 8 = 480 bytes at 4096; acc holds rows * ng = 24 doubles, 192 bytes
    assert call(acc=(C.c_void_p * 1)(4096 + 472)) == -1 and b"overlaps src" in err()
    assert call(acc=(C.c_void_p * 1)(4096 - 184)) == -1 and b"overlaps src" in err()
    assert call(acc=(C.c_void_p * 1)(4096 - 96)) == -1 and b"overlaps src" in err()     # would be clear with rows elements
    assert call(acc=(C.c_void_p * 1)(4096 + 480)) == -2 and call(acc=(C.c_void_p * 1)(4096 - 192)) == -2   # touching is fine
    two = dict(nf=2, src=(C.c_void_p * 2)(4096, 8192), sdt=(C.c_int * 2)(0, 1))
    assert call(acc=(C.c_void_p * 2)(1 << 20, (1 << 20) + 184), **two) == -1 and b"overlaps acc" in err()
    assert call(acc=(C.c_void_p * 2)(1 << 20, (1 << 20) + 192), **two) == -2
    # well-formed: only now is the device touched
    assert call() == -2 and call(flags=_gclim.ACCUMULATE) == -2 and call(w=None) == -2
    assert call(nt=2, t0=3) == -2 and call(ng=64) == -2


# ---- gclim_tables.hpp on its own, under the sanitizers -----------------------------------------------------------------
def test_gclim_tables_ranges_present_lists_and_shapes(tmp_path):
    """tests/host/gclim_tables_main.cpp: records of 1..600 times, ng in {1, 2, 5, 12, 64}, random and contiguous labels;
    every labelled time of a window in exactly one group range in ascending order, left-out times in none, the present
    list exact, the LDS bytes inside the budget, the launch shape a function of (nt, element size, groups present)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")
    exe = str(tmp_path / "gclim_tables_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                    os.path.join(ROOT, "tests", "host", "gclim_tables_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"records=(\d+) windows=(\d+) refusals=(\d+)", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) == 600 * 5 * 2 and int(m.group(2)) > 10 ** 6 and int(m.group(3)) == 11
    # neither header needs HIP
    for name in ("gclim_tables.hpp", "field_args.hpp"):
        hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", name)).read()
        assert not re.search(r"#include\s*<hip", hpp), name


# ---- front-end refusals before the device -------------------------------------------------------------------------------
def _tiny(nt=4):
    la = -90 + (np.arange(6) + 0.5) * 30.0
    lat = np.repeat(la, 8)
    plev = np.array([100.0, 500.0, 1000.0])
    f = np.zeros((lat.size, 3, nt))
    return lat, plev, f


BAD_GROUPS = [
    (dict(time_groups=[0, 1, 0, 1], climatology=False), "climatology=True"),
    (dict(time_weights=[1, 1, 1, 1]), "climatology=True"),
    (dict(time_groups=[0, 1, 0, 1], climatology=True, missing="mask", min_time_coverage=0.5), "missing='mask'"),
    (dict(time_weights=[1, 1, 1, 1], climatology=True, missing="mask", min_time_coverage=0.5), "missing='mask'"),
    (dict(time_groups=[0, 1, 0], climatology=True), "3 entries"),
    (dict(time_groups=[0, 1, 0, 1, 1], climatology=True), "5 entries"),
    (dict(time_weights=[1, 1, 1], climatology=True), "time_weights has shape"),
    (dict(time_groups=[0, 1, -2, 1], climatology=True), "labels are -1"),
    (dict(time_groups=[0.0, 1.0, 0.0, 1.0], climatology=True), "integer"),
    (dict(time_groups=[0, 2, 0, 2], climatology=True), "group 1 has no weight"),
    (dict(time_groups=[0, 1, 0, 1], time_weights=[1, 0, 1, 0], climatology=True), "group 1 has no weight"),
    (dict(time_groups=[-1, -1, -1, -1], climatology=True), "no time belongs"),
    (dict(time_groups=[0, 64, 1, 2], climatology=True), "65 groups"),
    (dict(time_weights=[1, -1, 1, 1], climatology=True), "finite and not negative"),
    (dict(time_weights=[1, np.nan, 1, 1], climatology=True), "finite and not negative"),
    (dict(time_groups="month", climatology=True), "datetime64"),
    (dict(time_groups="season", climatology=True, time=np.arange(4.0)), "datetime64"),
    (dict(time_groups="week", climatology=True, time=np.arange("2001-01", "2001-05", dtype="datetime64[M]")), "'month', 'season' or 'year'"),
]


@pytest.mark.parametrize("kw,match", BAD_GROUPS, ids=[str(i) for i in range(len(BAD_GROUPS))])
def test_group_keywords_are_refused_before_device(kw, match):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match=match):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, device=99, **kw)
    with pytest.raises(ValueError, match=match):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=plev, ps=np.zeros((lat.size, 4)), hyam=np.zeros(3),
                                         hybm=np.ones(3), device=99, **kw)
    # time-major model levels: the same refusals, before the record goes anywhere
    tm = np.zeros((4, 3, lat.size))
    with pytest.raises(ValueError, match=match):
        TEMDiagnostics.from_model_levels(tm, tm, tm, tm, lat, plev=plev, ps=np.zeros((4, lat.size)), hyam=np.zeros(3),
                                         hybm=np.ones(3), dims=("time", "lev", "ncol"), device=99, **kw)


@pytest.mark.parametrize("bad", [1, 0, "yes", None])
def test_climatology_stays_a_strict_bool_next_to_the_group_keywords(bad):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match="climatology must be True or False"):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, climatology=bad, time_groups=[0, 1, 0, 1], device=99)


def test_group_keywords_are_keyword_only_and_off_by_default():
    import inspect
    from pytemdiags_amd import TEMDiagnostics, climatology
    for name in ("time_groups", "time_weights"):
        p = inspect.signature(TEMDiagnostics.__init__).parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, name
    assert set(climatology.GROUP_SUM_KERNEL) == {"float64", "float32"}
    assert all(isinstance(v, bool) for v in climatology.GROUP_SUM_KERNEL.values())
    assert issubclass(climatology.GroupedBuilder, climatology.Builder)
    assert climatology.check_flag(True, "raise") is True          # check_flag keeps its behaviour
    with pytest.raises(ValueError):
        climatology.check_flag(True, "mask")


def test_resolved_groups_counts_weights_and_times():
    from pytemdiags_amd import climatology
    g = climatology.resolve_groups(LABELS, WEIGHTS, 7, np.arange(7.0))
    assert g.ng == 2 and g.names == [0, 1] and g.labels.dtype == np.int32
    np.testing.assert_array_equal(g.counts, [2, 4])
    np.testing.assert_array_equal(g.wsum, [0.75, 4.0])
    np.testing.assert_allclose(g.time, [(0.5 * 1 + 0.25 * 4) / 0.75, (0 + 2 * 3 + 5 + 0) / 4.0], rtol=1e-15)
    wm, wsum = weight_matrix(LABELS, WEIGHTS, 7)
    np.testing.assert_array_equal(g.matrix(), wm)
    np.testing.assert_array_equal(g.wsum, wsum)
    one = climatology.resolve_groups(None, [31, 28, 31], 3, np.array(["2001-01-16", "2001-02-15", "2001-03-16"], dtype="datetime64[D]"))
    assert one.ng == 1 and one.wsum[0] == 90 and one.weights.dtype == np.float64
    assert one.time[0] == np.datetime64("2001-02-15")          # (31 * 0 + 28 * 30 + 31 * 59) / 90 = 29.66 days on
    plain = climatology.resolve_groups(np.zeros(5, dtype=int), None, 5, np.arange(5))
    assert plain.weights is None and plain.wsum[0] == 5 and plain.time[0] == 2.0


def test_calendar_groups_on_two_years_of_days_starting_in_february():
    from pytemdiags_amd.climatology import calendar_groups
    t = np.arange("2001-02-01", "2003-02-01", dtype="datetime64[D]")
    month = t.astype("datetime64[M]").astype(int) % 12
    year = t.astype("datetime64[Y]").astype(int) + 1970
    lab, names = calendar_groups(t, "month")
    assert names == ["Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec"]
    assert lab.dtype == np.int32 and np.array_equal(lab, month)
    lab, names = calendar_groups(t, "season")
    assert names == ["DJF", "MAM", "JJA", "SON"]
    assert np.array_equal(lab, np.array([0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 0])[month])
    dec1, jan2 = (t == np.datetime64("2001-12-15")), (t == np.datetime64("2002-01-15"))
    assert lab[dec1][0] == lab[jan2][0] == 0
    lab, names = calendar_groups(t, "year")
    assert names == ["2001", "2002", "2003"] and np.array_equal(lab, year - 2001)
    # the groups are the keys present, in calendar order: a record of June to September has two seasons, JJA first
    part = np.arange("2001-06-01", "2001-10-01", dtype="datetime64[D]")
    lab, names = calendar_groups(part, "season")
    assert names == ["JJA", "SON"] and lab[0] == 0 and lab[-1] == 1
    lab, names = calendar_groups(part[::-1], "month")
    assert names == ["Jun", "Jul", "Aug", "Sep"] and lab[0] == 3 and lab[-1] == 0
    for bad in (np.arange(5.0), None, np.zeros((2, 2), dtype="datetime64[D]")):
        with pytest.raises(ValueError, match="datetime64"):
            calendar_groups(bad, "month")


def test_group_sum_gate_is_backed_by_a_committed_measurement():
    """``climatology.GROUP_SUM_KERNEL`` switches the kernel on for a dtype exactly where
    profiles/gclim_bench_mi355x.json shows it faster than the torch composition at ne120 x 72 x 30, two groups."""
    import json
    from pytemdiags_amd import climatology
    path = os.path.join(ROOT, "profiles", "gclim_bench_mi355x.json")
    assert os.path.exists(path), "GROUP_SUM_KERNEL without a measurement"
    legs = json.load(open(path))["time_sum_groups"]
    for name, on in climatology.GROUP_SUM_KERNEL.items():
        leg = [r for r in legs if (r["ncol"], r["nlev"], r["nt"], r["dtype"]) == (777602, 72, 30, name)]
        assert len(leg) == 1, name
        assert on == (leg[0]["torch_over_kernel_time"] > 1.0), (name, leg[0])
    # the legs the measurement has to hold
    have = {(r["ncol"], r["nlev"], r["nt"], r["dtype"], r["groups"]) for r in legs}
    assert {(777602, 72, 30, "float64", "2 contiguous"), (777602, 72, 30, "float32", "2 contiguous"),
            (48602, 72, 730, "float64", "24 contiguous"), (48602, 72, 730, "float64", "4 seasonal")} <= have


# ---- the construction, in numpy only -----------------------------------------------------------------------------------
def test_grouped_split_in_numpy_two_routes_shares_and_linear_results():
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(4)[:2]
    plev = synth.pressure_levels(6)
    f = synth.analytic_fields(lat, lon, plev, 7, seed=5)
    ref = gclim_reference(f, lat, plev, 20, LABELS, WEIGHTS, key="cs4-host")
    stat, zm = ref["stat"], ref["zm"]
    assert ref["wsum"].tolist() == [0.75, 4.0]
    # the group-mean state by the two routes: the operator is linear and does not depend on time
    for n in ZM7[:4]:
        assert getattr(stat, n).shape == zm["total"][n].shape == (180, 6, 2)
        e = np.abs(getattr(stat, n) - zm["total"][n]).max() / np.abs(zm["total"][n]).max()
        print("%s: two routes %.2e" % (n, e))
        assert e <= 1e-12, (n, e)
    # there is a transient part to speak of in every group
    for n in FLUXES:
        for g in range(2):
            share = np.abs(zm["transient"][n][..., g]).max() / np.abs(zm["total"][n][..., g]).max()
            print("%s group %d: transient share %.3f" % (n, g, share))
            assert share > 1e-3, (n, g, share)
    # the stationary run of both groups at once equals the runs one group at a time
    ff = [np.asarray(x, dtype=np.float64) for x in f]
    for g in range(2):
        alone = orc.TEMOracle(*[group_mean(x, ref["wm"][:, g:g + 1], ref["wsum"][g:g + 1]) for x in ff], lat, plev, L=20,
                              mode="factorised")
        for n in ZM7:
            a, b = getattr(alone, n)[..., 0], getattr(stat, n)[..., g]
            e = np.abs(a - b).max() / np.abs(b).max()
            assert e <= 1e-12, (n, g, e)
    # stationary + transient = total per group for the four results that are linear and homogeneous in the fluxes
    S, T, tot = (ref["sets"][k] for k in ("stationary", "transient", "total"))
    for n in LINEAR:
        for g in range(2):
            t = getattr(tot, n)()[..., g]
            e = np.abs(getattr(S, n)()[..., g] + getattr(T, n)()[..., g] - t).max() / np.abs(t).max()
            print("%s group %d: S + T - total %.2e" % (n, g, e))
            assert e <= 1e-12, (n, g, e)
    # a left-out time does not reach the reference, whatever it holds
    ff[0] = ff[0].copy()
    ff[0][..., 2] = np.nan
    wm, wsum = ref["wm"], ref["wsum"]
    assert np.array_equal(group_mean(ff[0], wm, wsum), group_mean(np.asarray(f[0], dtype=np.float64), wm, wsum))
