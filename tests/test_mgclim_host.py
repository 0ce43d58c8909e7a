"""Masked grouped time means, host side: the ctypes table against pytemdiags_amd/include/temx_mgclim.h and the plain-C
link check, the argument checks of temxw_time_sum_groups_valid before any device call, the launch shapes
(pytemdiags_amd/csrc/mgclim_shapes.hpp, which needs no HIP) on their own under AddressSanitizer + UBSan against their
mirrors in ``_mgclim``, the front end's refusals before any device call, and the numpy reference of the masked grouped
climatology with its self-checks.  Needs no GPU.

Bounds of the reference's self-checks, those the host files of the two parents hold between two numpy routes: on
NaN-free input it equals ``test_gclim_host.gclim_reference`` to 1e-12 of each quantity's maximum (on the 24 x 16 lat-lon
grid at L = 12, where tests/test_missing_host.py holds the masked oracle's lstsq to the default pipeline at that bound);
with one group of all times and no weights it equals ``test_nclim_host.masked_clim_reference`` to 1e-12, NaN patterns
and counts exactly."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import tem_oracle as orc
from test_gclim_host import BAD_GROUPS, FLUXES, LABELS, WEIGHTS, ZM7, gclim_reference
from test_missing_host import MaskedOracle, surface_mask
from test_nclim_host import masked_clim_reference, times_needed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pytemdiags_amd", "include", "temx_mgclim.h")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
SETS = ("total", "stationary", "transient")
_refs = {}


# ---- the reference of a masked grouped climatology, in numpy (shared with tests/test_gpu_mgclim_front.py) ------------
def counted_group_mean(x, valid, labels, w, need):
    """Per group g the weighted mean over the valid entries of the last axis labelled g: ``sum w x / sum w``, NaN where
    fewer than ``need[g]`` are valid or their weights sum to zero -> (means ``(..., G)``, counts ``(..., G)``)."""
    G = need.size
    mean = np.full(x.shape[:-1] + (G,), np.nan)
    cnt = np.zeros(x.shape[:-1] + (G,))
    for g in range(G):
        idx = np.nonzero(labels == g)[0]
        ok = valid[..., idx]
        cnt[..., g] = ok.sum(axis=-1)
        s = np.sum(np.where(ok, x[..., idx], 0.0) * w[idx], axis=-1)
        ws = np.sum(np.where(ok, w[idx], 0.0), axis=-1)
        with np.errstate(all="ignore"):
            mean[..., g] = np.where((cnt[..., g] >= need[g]) & (ws > 0), s / ws, np.nan)
    return mean, cnt


def masked_grouped_reference(fields, lat, plev, L, labels, weights, min_coverage, v, key=None):
    """-> dict: ``full`` the per-snapshot MaskedOracle, ``means`` the four counted, weighted and thresholded group-mean
    fields (ncol, nlev, G) with ``count`` their common count, ``stat`` the MaskedOracle of those at nt = G, ``n`` the
    times of each group and ``need`` the valid times a point needs, ``zcount`` the count of finite snapshots per group on
    the zonal grid, ``time_coverage`` = zcount / n, ``zm`` the seven zonal means of each set, ``sets`` the epilogue
    oracle of each and ``values`` their 26 quantities.  Computed once per ``key``, shared, left unchanged."""
    if key is not None and key in _refs:
        return _refs[key]
    f = [np.asarray(x, dtype=np.float64) for x in fields]
    N, nlev, nt = f[0].shape
    labels = np.asarray(labels)
    w = np.ones(nt) if weights is None else np.asarray(weights, dtype=np.float64)
    G = int(labels.max()) + 1
    n = np.array([(labels == g).sum() for g in range(G)])
    need = np.array([times_needed(v, k) for k in n])
    full = MaskedOracle(*f, lat, plev, L, min_coverage=min_coverage)
    valid = ~full.miss.reshape(N, nlev, nt)                                  # the common mask of the four
    means, count = [], None
    for x in f:
        m, count = counted_group_mean(x, valid, labels, w, need)
        means.append(m)
    stat = MaskedOracle(*means, lat, plev, L, min_coverage=min_coverage)
    tm, zcount = {}, None
    for name in ZM7:
        z = full.zonal[name]
        tm[name], c = counted_group_mean(z, np.isfinite(z), labels, w, need)
        assert zcount is None or np.array_equal(c, zcount), name            # the seven share their NaN pattern
        zcount = c
    zm = {"total": dict(tm), "stationary": dict(tm), "transient": dict(tm)}
    for name in FLUXES:
        zm["stationary"][name] = stat.zonal[name]
        zm["transient"][name] = tm[name] - stat.zonal[name]
    with np.errstate(all="ignore"):
        sets = {k: orc.TEMOracle.from_zonal_means(z, full.plev) for k, z in zm.items()}
        values = {k: dict(o.results(), **o.zonal_attrs()) for k, o in sets.items()}
    ref = {"full": full, "means": means, "count": count, "stat": stat, "n": n, "need": need, "zcount": zcount,
           "time_coverage": zcount / n.astype(np.float64), "zm": zm, "sets": sets, "values": values}
    if key is not None:
        _refs[key] = ref
    return ref


FRONT_PLEV = np.array([50.0, 150.0, 300.0, 500.0, 850.0, 995.0])


def front_mask(lat, lon, plev, nt):
    """A mask generator of this file's own (``surface_mask`` at 6 levels x 7 times leaves 70 % of the zonal points finite,
    the reference's self-check below asks for 90 %): below-ground points of a synthetic surface pressure with a small
    southern polar cap at 900 hPa, a plateau at 700 hPa and +-15 hPa of variation with time elsewhere, so that only the
    lowest level moves in and out of the ground.  True = missing, shape (ncol, nlev, nt)."""
    la, lo = np.asarray(lat)[:, None], np.asarray(lon)[:, None]
    t = np.arange(nt)[None, :]
    ps = 1000.0 + 15.0 * np.sin(np.deg2rad(lo) + 0.7 * t) * np.cos(np.deg2rad(la))
    ps = np.where(la < -80.0, 900.0, ps)
    plateau = (np.abs(la - 33.0) < 8.0) & (np.abs(lo - 88.0) < 15.0)
    ps = np.where(plateau, 700.0, ps)
    return np.asarray(plev)[None, :, None] > ps[:, None, :]


def front_fixture(dtype=np.float64, nan_free=False):
    """The fixture of the front-end tests: cs4 (866 columns) x 6 levels x 7 times under ``front_mask``.
    -> (lat, plev, fields); the fields are read-only."""
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(4)[:2]
    nt = 7
    f = [x.astype(dtype) for x in synth.analytic_fields(lat, lon, FRONT_PLEV, nt, seed=1)]
    if not nan_free:
        miss = front_mask(lat, lon, FRONT_PLEV, nt)
        f = [np.where(miss, np.nan, x).astype(dtype) for x in f]
    for x in f:
        x.setflags(write=False)
    return lat, FRONT_PLEV.copy(), f


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_mgclim_header_declares_exactly_what_is_bound():
    import ctypes as C
    from pytemdiags_amd import _lib, _mgclim
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(temxw_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _mgclim.SIGNATURES} == {"temxw_version", "temxw_time_sum_groups_valid"}
    assert not re.findall(r"\b(temx[vlicnmg]?_[a-z0-9_]+)\s*\(", code)   # the other headers' ABI is not extended from here
    lib = _mgclim.load()
    assert lib is _lib.load() and lib.temxw_version() == _mgclim.MGCLIM_VERSION == 100
    for name, value in (("TEMXW_NF_MAX", _mgclim.NF_MAX), ("TEMXW_NG_MAX", _mgclim.NG_MAX),
                        ("TEMXW_ACCUMULATE", _mgclim.ACCUMULATE), ("TEMXW_COMMON_MASK", _mgclim.COMMON_MASK)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const void* const*": C.POINTER(C.c_void_p),
             "double* const*": C.POINTER(C.c_void_p), "const int32_t*": C.POINTER(C.c_int32),
             "const double*": C.POINTER(C.c_double)}
    sig = dict((n, (r, a)) for n, r, a in _mgclim.SIGNATURES)
    decl = re.search(r"int temxw_time_sum_groups_valid\((.*?)\);", code, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert sig["temxw_time_sum_groups_valid"] == (C.c_int, [ctype[p.rsplit(" ", 1)[0]] for p in params])
    assert sig["temxw_version"] == (C.c_int, [])
    assert [p.rsplit(" ", 1)[1] for p in params] == [
        "device", "nf", "src_host", "src_dtype", "acc_host", "wsum_host", "cnt_host", "ncol", "nlev", "nt", "nt_record", "t0",
        "ng", "label_host", "weight_host_or_null", "flags", "stream"]
    # the entry point is a function-try-block, like every other one; the other versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    assert re.search(r"^int temxw_time_sum_groups_valid\([^;{]*\)\s*try \{\s*$", src, re.M)
    for fn, v in (("temx", 402), ("temxv", 100), ("temxl", 100), ("temxi", 100), ("temxc", 100), ("temxm", 100),
                  ("temxn", 100), ("temxg", 100), ("temxw", 100)):
        assert "int %s_version(void) { return %d; }" % (fn, v) in src, fn
    # the eight headers of include/ declare nothing of this feature
    for n in os.listdir(os.path.join(ROOT, "include")):
        assert "temxw_" not in open(os.path.join(ROOT, "include", n)).read(), n
    mk = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "Makefile")).read()
    assert "../include/temx_mgclim.h" in mk


def test_mgclim_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_mgclim")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_mgclim.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxw_version=100 nf0_rc=-1 ng65_rc=-1" in out.stdout
    assert "temx_version=402" in out.stdout


def test_time_sum_groups_valid_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _mgclim
    lib = _mgclim.load()
    one = lambda p: (C.c_void_p * 1)(p)
    src, acc, wsum, cnt = one(4096), one(1 << 20), one(2 << 20), one(3 << 20)
    lab5 = (C.c_int32 * 5)(0, 1, -1, 1, 0)
    w5 = (C.c_double * 5)(1.0, 0.5, 3.0, 2.0, 0.0)

    def call(nf=1, src=src, dt=0, acc=acc, wsum=wsum, cnt=cnt, ncol=4, nlev=3, nt=5, ntr=5, t0=0, ng=2, lab=lab5, w=w5,
             flags=_mgclim.COMMON_MASK):
        # device 99 does not exist: a call that got as far as the device would come back TEMX_EHIP, not TEMX_EINVAL
        return lib.temxw_time_sum_groups_valid(99, nf, src, dt, acc, wsum, cnt, ncol, nlev, nt, ntr, t0, ng, lab, w, flags, None)
    err = lib.temx_last_error
    assert call(nf=0) == -1 and b"nf" in err()
    assert call(nf=9) == -1
    for name in ("src", "acc", "wsum", "cnt"):
        assert call(**{name: None}) == -1 and name.encode() in err(), name
        assert call(**{name: one(None)}) == -1 and b"null" in err(), name
    assert call(dt=2) == -1 and b"dtype" in err()
    assert call(flags=4) == -1 and b"flags" in err()
    assert call(ncol=0) == -1 and call(nlev=0) == -1 and call(nt=0) == -1
    assert call(src=one(4100)) == -1 and b"aligned" in err()                  # fp64 at 4 mod 8
    assert call(src=one(4100), dt=1) == -2                                    # fp32 at 4 mod 8 is aligned
    for name in ("acc", "wsum", "cnt"):
        assert call(**{name: one((5 << 20) + 4)}) == -1 and b"aligned" in err() and name.encode() in err(), name
    # the group arguments
    assert call(ng=0) == -1 and b"ng must lie in 1..64" in err()
    assert call(ng=65) == -1 and b"ng must lie in 1..64" in err()
    assert call(t0=-1, nt=2) == -1 and b"t0 must not be negative" in err()
    assert call(t0=1) == -1 and b"exceeds nt_record" in err()
    assert call(nt=6) == -1 and b"exceeds nt_record" in err()
    assert call(lab=None) == -1 and b"label_host" in err()
    assert call(lab=(C.c_int32 * 5)(0, 1, -2, 1, 0)) == -1 and b"label 2 is -2" in err()
    assert call(ng=1) == -1 and b"label 1 is 1" in err()
    for v in (-0.5, float("nan"), float("inf")):
        assert call(w=(C.c_double * 5)(1.0, 0.5, v, 2.0, 0.0)) == -1 and b"weight 2 must be finite and not negative" in err()
    # src is 4 * 3 * 5 * 8 = 480 bytes at 4096; an output holds rows * ng = 24 doubles, 192 bytes
    for name in ("acc", "wsum", "cnt"):
        assert call(**{name: one(4096 + 472)}) == -1 and ("%s 0 overlaps src 0" % name).encode() in err(), name
        assert call(**{name: one(4096 - 184)}) == -1 and ("%s 0 overlaps src 0" % name).encode() in err(), name
        assert call(**{name: one(4096 + 480)}) == -2 and call(**{name: one(4096 - 192)}) == -2, name     # touching is fine
    assert call(wsum=one((1 << 20) + 184)) == -1 and b"wsum 0 overlaps acc 0" in err()
    assert call(cnt=one((1 << 20) - 184)) == -1 and b"cnt 0 overlaps acc 0" in err()
    assert call(wsum=one((3 << 20) + 8)) == -1 and b"wsum 0 overlaps cnt 0" in err()
    assert call(wsum=one((1 << 20) + 192), cnt=one((1 << 20) + 384)) == -2
    # own masks: every field's wsum and cnt is used; under a common mask only the first
    two = dict(nf=2, src=(C.c_void_p * 2)(4096, 8192), acc=(C.c_void_p * 2)(1 << 20, (1 << 20) + 192))
    assert call(wsum=(C.c_void_p * 2)(2 << 20, None), cnt=(C.c_void_p * 2)(3 << 20, None), **two) == -2
    assert call(wsum=(C.c_void_p * 2)(2 << 20, None), cnt=(C.c_void_p * 2)(3 << 20, 4 << 20), flags=0, **two) == -1
    assert b"wsum 1 is null" in err()
    assert call(wsum=(C.c_void_p * 2)(2 << 20, 4 << 20), cnt=(C.c_void_p * 2)(3 << 20, None), flags=0, **two) == -1
    assert b"cnt 1 is null" in err()
    assert call(wsum=(C.c_void_p * 2)(2 << 20, (2 << 20) + 184), cnt=(C.c_void_p * 2)(3 << 20, 4 << 20), flags=0, **two) == -1
    assert b"wsum 1 overlaps wsum 0" in err()
    assert call(acc=(C.c_void_p * 2)(1 << 20, (1 << 20) + 184), nf=2, src=two["src"]) == -1 and b"overlaps acc" in err()
    assert call(wsum=(C.c_void_p * 2)(2 << 20, 4 << 20), cnt=(C.c_void_p * 2)(3 << 20, 5 << 20), flags=0, **two) == -2
    # well-formed: only now is the device touched
    assert call() == -2 and call(flags=_mgclim.ACCUMULATE) == -2 and call(w=None) == -2 and call(flags=3) == -2
    assert call(nt=2, t0=3) == -2 and call(ng=64) == -2


# ---- mgclim_shapes.hpp on its own, under the sanitizers, against the mirrors of _mgclim -------------------------------
def test_mgclim_shapes_units_owned_once_lds_budgets_batches_and_switch_points(tmp_path):
    """tests/host/mgclim_shapes_main.cpp: nt = 1..2000, both dtypes, 1..8 fields per workgroup, 1..64 groups present, a
    few row counts."""
    from pytemdiags_amd import _gclim, _mgclim, _nclim
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")
    exe = str(tmp_path / "mgclim_shapes_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                    os.path.join(ROOT, "tests", "host", "mgclim_shapes_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"cases=(\d+) walked=(\d+)", out.stdout)
    assert int(m.group(1)) > 2 * 10 ** 6
    # ownership is walked at every nt: at least one row count and np in {1, 5, 64} for each (dtype, fields, nt)
    assert int(m.group(2)) >= 2 * 8 * 2000 * 3
    assert "refusals=20" in out.stdout                 # check_sum_groups_valid of field_args.hpp, every refusal
    # the mirrors: the switch to the long rows is the grouped sum's, whatever the fields; the batch of the LDS form
    sw = {int(e): int(n) for e, n in re.findall(r"switch esz=(\d+) nt=(\d+)", out.stdout)}
    assert sw == {8: 256, 4: 512}
    for esz in (8, 4):
        for nf in (1, 4, 8):
            for common in (False, True):
                assert _mgclim.switch_nt(esz, nf, common) == sw[esz] == _gclim.switch_nt(esz)
    slots = {int(n): int(b) for n, b in re.findall(r"batch nfs=(\d+) slots=(\d+)", out.stdout)}
    assert slots == {n: _mgclim.batch(n) for n in range(1, 9)} and slots[8] == 12 and slots[4] == 21 and slots[1] == 42
    assert [_mgclim.bound(n) for n in (1, 2, 4, 5, 64)] == [1, 4, 4, 64, 64]
    # the shape itself, at the points where it changes
    s = _mgclim.shape(111, 30, 8, 4, 2)
    assert (s["staged"], s["rpb"], s["stride"], s["lds_bytes"]) == (1, 33, 31, 4 * 33 * 31 * 8) and s["nblk"] == 4
    few = _nclim.switch_nt(8, 4, True)
    assert few == 64 and _mgclim.shape(111, few - 1, 8, 4, 2)["rpb"] == 16 and _mgclim.shape(111, few, 8, 4, 2)["rpb"] == 15
    assert _mgclim.shape(111, 255, 8, 8, 2) == dict(staged=1, rpb=2, stride=255, bound=0, batch=0, npass=1, rpw=2,
                                                    lds_bytes=8 * 2 * 255 * 8, nblk=56)
    assert _mgclim.shape(111, 256, 8, 8, 2) == dict(staged=0, rpb=0, stride=0, bound=4, batch=0, npass=1, rpw=4, lds_bytes=0,
                                                    nblk=28)
    assert _mgclim.shape(111, 256, 8, 8, 12) == dict(staged=0, rpb=0, stride=0, bound=64, batch=12, npass=1, rpw=1,
                                                     lds_bytes=61440, nblk=111)
    assert _mgclim.shape(111, 256, 8, 8, 13)["npass"] == 2 and _mgclim.shape(111, 256, 8, 4, 22)["npass"] == 2
    assert _mgclim.shape(111, 730, 8, 4, 12)["rpw"] == 1 and _mgclim.shape(111, 730, 8, 4, 5)["rpw"] == 4
    for name in ("mgclim_shapes.hpp", "gclim_tables.hpp", "nclim_shapes.hpp"):
        hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", name)).read()
        assert not re.search(r"#include\s*<hip", hpp), name
    hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "mgclim_shapes.hpp")).read()
    assert re.search(r"MGCLIM_LONG_LDS_BYTES = 64 \* 1024;", hpp) and _mgclim.LONG_LDS_BYTES == 64 * 1024


# ---- front-end refusals before the device ----------------------------------------------------------------------------
def _tiny(nt=4):
    la = -90 + (np.arange(6) + 0.5) * 30.0
    lat = np.repeat(la, 8)
    plev = np.array([100.0, 500.0, 1000.0])
    f = np.zeros((lat.size, 3, nt))
    return lat, plev, f


def test_min_group_coverage_refusals_come_before_the_device():
    from pytemdiags_amd import TEMDiagnostics, climatology
    lat, plev, f = _tiny()
    tm = np.zeros((4, 3, lat.size))

    def direct(**kw):
        return TEMDiagnostics(f, f, f, f, lat, plev=plev, device=99, **kw)

    def levels(**kw):
        return TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=plev, ps=np.zeros((lat.size, 4)), hyam=np.zeros(3),
                                                hybm=np.ones(3), device=99, **kw)

    def time_major(**kw):
        return TEMDiagnostics.from_model_levels(tm, tm, tm, tm, lat, plev=plev, ps=np.zeros((4, lat.size)), hyam=np.zeros(3),
                                                hybm=np.ones(3), dims=("time", "lev", "ncol"), device=99, **kw)
    g = dict(time_groups=[0, 1, 0, 1])
    for build in (direct, levels, time_major):
        # without climatology=True and missing="mask", or without any of the group keywords
        for kw in (dict(g, min_group_coverage=0.5), dict(g, climatology=True, min_group_coverage=0.5),
                   dict(g, missing="mask", min_group_coverage=0.5), dict(climatology=True, missing="mask", min_group_coverage=0.5)):
            with pytest.raises(ValueError, match="min_group_coverage belongs to the masked grouped means"):
                build(**kw)
        # together with min_time_coverage
        with pytest.raises(ValueError, match="min_group_coverage and min_time_coverage exclude each other"):
            build(climatology=True, missing="mask", min_group_coverage=0.5, min_time_coverage=0.5, **g)
        # outside (0, 1] or not a number
        for bad in (0, 0.0, -0.5, 1.0000001, 2, "half", float("nan"), True, (0.5,)):
            with pytest.raises(ValueError, match="min_group_coverage must be a number"):
                build(climatology=True, missing="mask", min_group_coverage=bad, **g)
        # without the keyword the old refusals stand, with their messages
        with pytest.raises(ValueError, match="masked grouped means are not served"):
            build(climatology=True, missing="mask", min_time_coverage=0.5, **g)
        with pytest.raises(ValueError, match="a contract of its own"):
            build(climatology=True, missing="mask")
        # every min_time_coverage refusal, through the new signature with the new keyword off
        none = dict(min_group_coverage=None)
        for bad in (0, 0.0, -0.5, 1.0000001, 2, "half", float("nan"), True, (0.5,)):
            with pytest.raises(ValueError, match="min_time_coverage must be a number"):
                build(climatology=True, missing="mask", min_time_coverage=bad, **none)
        for kw in (dict(climatology=True), dict(missing="mask"), dict()):
            with pytest.raises(ValueError, match="min_time_coverage belongs to the masked climatology"):
                build(min_time_coverage=0.5, **kw, **none)
        with pytest.raises(ValueError, match="a contract of its own"):
            build(climatology=True, missing="mask", **none)
        # with it, the record is still checked on the host
        with pytest.raises(ValueError, match="3 entries"):
            build(climatology=True, missing="mask", min_group_coverage=0.5, time_groups=[0, 1, 0])
        with pytest.raises(ValueError, match="group 1 has no weight"):
            build(climatology=True, missing="mask", min_group_coverage=0.5, time_weights=[1, 0, 1, 0], **g)
    # a good value gets past the checks: what stops the run now is the device that does not exist
    for v in (0.5, 1, 1.0, 1e-6, np.float32(0.25)):
        for kw in (g, dict(time_weights=[1, 2, 3, 4]), dict(g, time_weights=[1, 2, 3, 4])):
            with pytest.raises(Exception) as ei:
                direct(climatology=True, missing="mask", min_group_coverage=v, **kw)
            assert not isinstance(ei.value, ValueError), (v, str(ei.value))
    assert climatology.check_group_coverage(None, False, "raise", None, None) is None
    assert climatology.check_group_coverage(0.25, True, "mask", [0], None) == 0.25
    assert climatology.group_times_needed(0.5, [2, 4, 5, 1]).tolist() == [1, 2, 3, 1]
    assert climatology.group_times_needed(0.6, [5]).tolist() == [3] and climatology.group_times_needed(1.0, [5]).tolist() == [5]


@pytest.mark.parametrize("kw,match", BAD_GROUPS, ids=[str(i) for i in range(len(BAD_GROUPS))])
def test_every_refusal_of_the_grouped_means_stands_without_the_keyword(kw, match):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match=match):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, device=99, min_group_coverage=None, **kw)


def test_min_group_coverage_is_keyword_only_and_off_by_default():
    import inspect
    from pytemdiags_amd import TEMDiagnostics, climatology
    p = inspect.signature(TEMDiagnostics.__init__).parameters["min_group_coverage"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert issubclass(climatology.MaskedGroupedBuilder, climatology.Builder)
    assert climatology.check_flag(True, "raise") is True
    with pytest.raises(ValueError):
        climatology.check_flag(True, "mask")
    with pytest.raises(ValueError, match="not served"):
        climatology.check_group_flags([0, 1], None, True, "mask")


# ---- the numpy reference: self-checks --------------------------------------------------------------------------------
def test_masked_grouped_reference_on_nan_free_input_is_the_grouped_reference():
    from pytemdiags_amd import synth
    from test_missing_host import latlon
    lat, lon = latlon(24, 16)
    plev = synth.pressure_levels(8)
    f = synth.analytic_fields(lat, lon, plev, 7, seed=5)
    ref = masked_grouped_reference(f, lat, plev, 12, LABELS, WEIGHTS, 0.5, 0.5)
    plain = gclim_reference(f, lat, plev, 12, LABELS, WEIGHTS)
    assert np.all(ref["time_coverage"] == 1.0) and np.all(ref["count"] == [2, 4]) and ref["need"].tolist() == [1, 2]
    want = {"total": plain["sets"]["total"], "stationary": plain["stat"], "transient": plain["sets"]["transient"]}
    worst = (0.0, "")
    for s in SETS:
        w = dict(want[s].results(), **want[s].zonal_attrs())
        assert len(w) == 26
        for n, r in w.items():
            assert r.shape == ref["values"][s][n].shape == (180, 8, 2)
            e = float(np.max(np.abs(ref["values"][s][n] - r)) / max(np.max(np.abs(r)), 1e-300))
            worst = max(worst, (e, "%s.%s" % (s, n)))
            assert e <= 1e-12, (s, n, e)
    print("masked grouped reference against the grouped one, NaN-free input: worst %.2e (%s)" % worst)


def test_masked_grouped_reference_with_one_group_is_the_masked_reference():
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(4)[:2]
    plev = np.sort(synth.pressure_levels(8) * 0.5 + 500.0 * np.linspace(0, 1, 8) ** 2)
    f = synth.analytic_fields(lat, lon, plev, 5, seed=1)
    miss = surface_mask(lat, lon, plev, 5)
    f = [np.where(miss, np.nan, x) for x in f]
    one = masked_grouped_reference(f, lat, plev, 20, np.zeros(5, dtype=int), None, 0.5, 0.5)
    old = masked_clim_reference(f, lat, plev, 20, 0.5, 0.5)
    assert one["need"].tolist() == [old["need"]] and np.array_equal(one["count"][..., 0], old["count"])
    assert np.array_equal(one["time_coverage"], old["time_coverage"]) and np.array_equal(one["zcount"][..., 0], old["zcount"])
    nans = 0
    for s in SETS:
        for n, r in old["values"][s].items():
            x = one["values"][s][n]
            assert np.array_equal(np.isnan(x), np.isnan(r)), (s, n)
            fin = np.isfinite(r)
            e = float(np.max(np.abs(x[fin] - r[fin])) / np.max(np.abs(r[fin])))
            assert e <= 1e-12, (s, n, e)
            nans += int(np.isnan(r).sum())
    assert nans


def test_the_reference_of_the_front_end_fixture_is_not_vacuous():
    """On the CPU, on the reference alone: counts and thresholds are both exercised in every group, most of the zonal
    grid is finite, and no coverage lies within 1e-6 of the threshold, so NaN patterns can be compared exactly."""
    lat, plev, f = front_fixture()
    ref = masked_grouped_reference(f, lat, plev, 20, LABELS, WEIGHTS, 0.5, 0.5, key="cs4-front")
    assert ref["n"].tolist() == [2, 4] and ref["need"].tolist() == [1, 2]
    c = ref["count"]
    for g in range(2):
        part = (c[..., g] > 0) & (c[..., g] < ref["n"][g])
        below, kept = c[..., g] < ref["need"][g], c[..., g] >= ref["need"][g]
        print("group %d: %d points with some times, %d below need, %d at or above" % (g, part.sum(), below.sum(), kept.sum()))
        assert part.any() and below.any() and kept.any(), g
        z = ref["zcount"][..., g]
        assert ((z > 0) & (z < ref["n"][g])).any(), g
    fin = np.ones((180, 6, 2), dtype=bool)
    for s in SETS:
        for n, r in ref["values"][s].items():
            fin &= np.isfinite(r)
    print("finite in all three sets: %.1f %% of the zonal points" % (100.0 * fin.mean()))
    assert fin.mean() >= 0.9
    d_snap = float(np.abs(ref["full"].coverage - 0.5).min())
    d_stat = float(np.nanmin(np.abs(ref["stat"].coverage - 0.5)))
    print("smallest distance of a coverage from 0.5: per snapshot %.2e, stationary %.2e" % (d_snap, d_stat))
    assert d_snap >= 1e-6 and d_stat >= 1e-6
