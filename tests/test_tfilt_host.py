"""EP flux by time scale, host side: the ctypes table against pytemdiags_amd/include/temx_tfilt.h and the plain-C link
check, the cut and the argument checker of the time filter (pytemdiags_amd/csrc/tfilt_shapes.hpp, which needs no HIP) on
their own under AddressSanitizer + UBSan and through the library on made-up addresses, the refusals of the front end that
are decided before any device call, and the Lanczos weights.  Needs no GPU."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pytemdiags_amd", "include", "temx_tfilt.h")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
EINVAL, EHIP, EUNSUPPORTED = -1, -2, -6


# ---- header and bindings ---------------------------------------------------------------------------------------------
def test_tfilt_header_declares_exactly_what_is_bound():
    from pytemdiags_amd import _lib, _tfilt
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(temxf_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _tfilt.SIGNATURES} == {"temxf_version", "temxf_filter_time", "temxf_filter_shape"}
    assert not re.findall(r"\b(temx[vlicnmgwk]?_[a-z0-9_]+)\s*\(", code)   # the other headers' ABI is not extended from here
    lib = _tfilt.load()
    assert lib is _lib.load() and lib.temxf_version() == _tfilt.TFILT_VERSION == 100
    for name, value in (("TEMXF_NF_MAX", _tfilt.NF_MAX), ("TEMXF_NB_MAX", _tfilt.NB_MAX), ("TEMXF_NW_MAX", _tfilt.NW_MAX)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    assert (_tfilt.NF_MAX, _tfilt.NB_MAX, _tfilt.NW_MAX) == (8, 4, 255)
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const double*": C.c_void_p,
             "const void* const*": C.POINTER(C.c_void_p), "void* const*": C.POINTER(C.c_void_p),
             "const int*": C.POINTER(C.c_int), "int*": C.POINTER(C.c_int)}
    sig = dict((n, (r, a)) for n, r, a in _tfilt.SIGNATURES)
    names = {"temxf_filter_time": ["device", "nf", "src_host", "src_dtype_host", "nb", "dst_host", "dst_dtype", "ncol", "nlev",
                                   "nt", "nw", "weights", "flags", "stream"],
             "temxf_filter_shape": ["rows", "nt", "nw", "nb", "src_esz", "dst_esz", "shape_host"]}
    for fn, want in names.items():
        decl = re.search(r"int %s\((.*?)\);" % fn, code, re.S).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert sig[fn] == (C.c_int, [ctype[p.rsplit(" ", 1)[0]] for p in params]), fn
        assert [p.rsplit(" ", 1)[1] for p in params] == want, fn
    assert sig["temxf_version"] == (C.c_int, [])
    # the entry points are function-try-blocks, like every other one; the other ten versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    for fn in names:
        assert re.search(r"^int %s\([^;{]*\)\s*try \{\s*$" % fn, src, re.M), fn
    for fn, v in (("temx", 402), ("temxv", 100), ("temxl", 100), ("temxi", 100), ("temxc", 100), ("temxm", 100),
                  ("temxn", 100), ("temxg", 100), ("temxw", 100), ("temxk", 100), ("temxf", 100)):
        assert "int %s_version(void) { return %d; }" % (fn, v) in src, fn
    # the other ten headers declare nothing of this feature; the Makefile knows the new one
    seen = 0
    for d in (os.path.join(ROOT, "include"), os.path.dirname(HEADER)):
        for n in os.listdir(d):
            if n != "temx_tfilt.h":
                seen += 1
                assert "temxf_" not in open(os.path.join(d, n)).read(), n
    assert seen == 10
    mk = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "Makefile")).read()
    assert "../include/temx_tfilt.h" in mk and "$(wildcard *.hpp)" in mk
    # the cut and the checker live in a header without HIP, and the kernel is the one temx.hip includes
    hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "tfilt_shapes.hpp")).read()
    assert not re.search(r"#include\s*[<\"]hip", hpp) and "TFILT_NW_MAX = %d" % _tfilt.NW_MAX in hpp
    assert '#include "kernels_tfilt.hpp"' in src and '#include "tfilt_shapes.hpp"' in src


def test_tfilt_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_tfilt")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_tfilt.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxf_version=100 even_rc=-1 short_rc=-1 narrow_rc=-1 null_rc=-1 shape_rc=0" in out.stdout
    assert "temx_version=402" in out.stdout


# ---- tfilt_shapes.hpp on its own, under the sanitizers ------------------------------------------------------------------
def test_tfilt_shapes_cut_and_checker_under_sanitizers(tmp_path):
    """tests/host/tfilt_shapes_main.cpp replays the index arithmetic of the kernel lane by lane over a sweep of sizes:
    every (row, output time) is stored exactly once, the staged image fits its budget, every read lies inside its row or
    its image, no grid dimension overflows; and it runs every refusal of the checker on made-up addresses."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")
    exe = str(tmp_path / "tfilt_shapes_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                    os.path.join(ROOT, "tests", "host", "tfilt_shapes_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"shapes=(\d+) refusals=(\d+) cut=ok checker=ok\s*$", out.stdout)
    assert m and "FAILED" not in out.stdout
    assert int(m.group(1)) > 1500 and int(m.group(2)) == 27


# ---- the checker through the library, on made-up addresses ---------------------------------------------------------------
NCOL, NLEV, NT, NW = 10, 2, 40, 9
SRC_BYTES = NCOL * NLEV * NT * 8
DST_BYTES = NCOL * NLEV * (NT - NW + 1) * 8
BASE = 1 << 20
SRC = [BASE, BASE + SRC_BYTES]
D0 = BASE + 2 * SRC_BYTES
DST = [D0 + i * DST_BYTES for i in range(4)]
W = D0 + 4 * DST_BYTES
F64, F32 = 0, 1


def _call(nf=2, src=SRC, dts=(F64, F64), nb=2, dst=DST, dd=F64, ncol=NCOL, nlev=NLEV, nt=NT, nw=NW, w=W, flags=0,
          null=None):
    from pytemdiags_amd import _tfilt
    lib = _tfilt.load()
    a_src = (C.c_void_p * len(src))(*src) if null != "src_host" else None
    a_dts = (C.c_int * len(dts))(*dts) if null != "src_dtype_host" else None
    a_dst = (C.c_void_p * len(dst))(*dst) if null != "dst_host" else None
    rc = lib.temxf_filter_time(99, nf, a_src, a_dts, nb, a_dst, dd, ncol, nlev, nt, nw, C.c_void_p(w), flags, None)
    return rc, lib.temx_last_error().decode()


REFUSED = [
    (dict(nf=0), "nf must lie"), (dict(nf=9), "nf must lie"), (dict(null="src_host"), "src_host is null"),
    (dict(null="src_dtype_host"), "src_dtype_host is null"), (dict(null="dst_host"), "dst_host is null"),
    (dict(w=None), "weights is null"), (dict(nb=0), "nb must lie"), (dict(nb=5), "nb must lie"),
    (dict(nw=0), "nw must lie"), (dict(nw=257, nt=400), "nw must lie"), (dict(nw=8), "nw must be odd"),
    (dict(nt=8), "shorter than the filter"), (dict(ncol=0), "ncol must be at least 1"), (dict(nlev=0), "nlev must be at least 1"),
    (dict(nt=0), "nt must be at least 1"), (dict(dts=(F64, 7)), "src_dtype 1 must be"), (dict(dd=5), "dst_dtype must be"),
    (dict(flags=1), "unknown bits"), (dict(dd=F32), "does not narrow"), (dict(src=[BASE, 0]), "src 1 is null"),
    (dict(src=[BASE, BASE + SRC_BYTES + 4]), "src 1 is not aligned"), (dict(dst=DST[:2] + [0, DST[3]]), "dst 2 (band 1, field 0) is null"),
    (dict(dst=DST[:2] + [DST[2] + 4, DST[3]]), "dst 2 (band 1, field 0) is not aligned"), (dict(w=W + 4), "weights is not aligned"),
    (dict(dst=DST[:3] + [SRC[1] + SRC_BYTES - 8]), "dst 3 overlaps src 1"), (dict(dst=DST[:3] + [DST[2] + DST_BYTES - 8]), "dst 3 overlaps dst 2"),
    (dict(w=DST[3] + DST_BYTES - 8), "dst 3 overlaps weights"),
]


@pytest.mark.parametrize("kw,match", REFUSED, ids=[m.replace(" ", "_") + str(i) for i, (_, m) in enumerate(REFUSED)])
def test_tfilt_checker_refuses_before_any_device_call(kw, match):
    rc, msg = _call(**kw)
    assert rc == EINVAL and match in msg, (rc, msg)


def test_tfilt_good_arguments_reach_the_device_call():
    """Device 99 does not exist: a call that passes every check fails at hipSetDevice (TEMX_EHIP), whatever the dtypes."""
    for kw in (dict(), dict(dts=(F32, F32), dd=F32), dict(dts=(F32, F64)), dict(nt=NW, nf=1, nb=1), dict(nw=1, nf=1, nb=1, src=[BASE], dts=(F64,), dst=[D0]),
               dict(src=[BASE, BASE + SRC_BYTES + 4], dts=(F64, F32))):
        rc, msg = _call(**kw)
        assert rc == EHIP, (kw, rc, msg)


def test_tfilt_shape_through_the_library():
    from pytemdiags_amd import _tfilt
    lib = _tfilt.load()
    s = _tfilt.shape(3499344, 730, 31, 2, 8, 8)
    assert s == dict(rpb=32, TT=128, stride=159, R=8, ntile=6, grid=6 * 109355, lds_bytes=32 * 159 * 8)
    assert _tfilt.shape(3499344, 730, 121)["rpb"] == 16 and _tfilt.shape(3499344, 730, 121, 1, 4, 4)["rpb"] == 32
    assert _tfilt.shape(1000, 3, 3)["rpb"] == 256 and _tfilt.shape(1, 3, 3)["grid"] == 1
    for rows, nt, nw in ((1, 300, 3), (1000, 40, 9), (7, 255, 255), (33, 1000, 255)):
        for se, de in ((8, 8), (4, 4), (4, 8)):
            s = _tfilt.shape(rows, nt, nw, 1, se, de)
            nto = nt - nw + 1
            assert s["stride"] % 2 == 1 and s["stride"] >= s["TT"] + nw - 1 and s["TT"] % s["R"] == 0
            assert s["lds_bytes"] == s["rpb"] * s["stride"] * se <= 40960
            assert s["ntile"] == -(-nto // s["TT"]) and s["grid"] == s["ntile"] * -(-rows // s["rpb"])
    out = (C.c_int * 7)()
    for args, code, match in (((0, 40, 9, 1, 8, 8), EINVAL, "at least 1"), ((10, 40, 8, 1, 8, 8), EINVAL, "odd"),
                              ((10, 8, 9, 1, 8, 8), EINVAL, "shorter"), ((10, 40, 9, 5, 8, 8), EINVAL, "nb must lie"),
                              ((10, 40, 9, 1, 2, 8), EINVAL, "4 or 8"), ((10, 40, 9, 1, 8, 4), EINVAL, "no fp32 destination"),
                              ((1 << 29, 80, 9, 1, 8, 8), EUNSUPPORTED, "in parts along ncol")):
        assert lib.temxf_filter_shape(*args, out) == code and match in lib.temx_last_error().decode(), args
    assert lib.temxf_filter_shape(10, 40, 9, 1, 8, 8, None) == EINVAL
    assert lib.temxf_filter_shape((1 << 29) - 32, 80, 9, 1, 8, 8, out) == 0 and out[5] == (1 << 24) - 1
    # the same limit refuses the launch itself, before any device call
    big = 1 << 29
    rc, msg = _call(nf=1, src=[8], dts=(F64,), nb=1, dst=[1 << 50], ncol=big, nlev=1, nt=80, w=1 << 60)
    assert rc == EUNSUPPORTED and "in parts along ncol" in msg, (rc, msg)


# ---- the oracle of the GPU tests, on its own --------------------------------------------------------------------------
def test_fraction_oracle_rounds_subnormals_signs_zeros_and_overflows_fp32():
    """``exact_fma`` and ``oracle`` of tests/test_gpu_tfilt.py against constants derived by hand (this Python has no
    ``math.fma``): ties to even in the subnormal range, the sign of an underflow, the signs of exact zeros under round to
    nearest, one rounding instead of two, and the final rounding to fp32 with its subnormals and its overflow to inf.
    The random pools give the numbers the plain Fraction chain gives."""
    from fractions import Fraction as Fr

    import test_gpu_tfilt as tf
    den = 2.0 ** -1074

    def fma(w, x, acc):
        return tf.exact_fma(Fr(w), Fr(x), acc, w, x)

    def same(a, b):
        return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)

    assert same(fma(0.5, den, 0.0), 0.0)                      # 2^-1075: a tie, to even
    assert same(fma(0.5, 3 * den, 0.0), 2 * den)              # 1.5 den: a tie, to even
    assert same(fma(0.75, den, 0.0), den) and same(fma(0.25, den, 0.0), 0.0)
    assert same(fma(-0.25, den, 0.0), -0.0) and same(fma(0.25, -den, 0.0), -0.0)          # an underflow keeps its sign
    assert same(fma(-0.75, den, 0.0), -den) and same(fma(0.5, 2.0 ** -1022, 0.0), 2.0 ** -1023)
    assert same(fma(1 + 2.0 ** -52, 1 + 2.0 ** -52, -(1 + 2.0 ** -51)), 2.0 ** -104)      # one rounding, not two
    assert same(fma(2.0 ** -537, 2.0 ** -537, den), 2 * den)  # the product alone underflows; the sum is exact
    assert same(fma(1.0, -0.0, 0.0), 0.0) and same(fma(1.0, -0.0, -0.0), -0.0) and same(fma(-1.0, 0.0, -0.0), -0.0)
    assert same(fma(-1.0, -0.0, -0.0), 0.0) and same(fma(0.0, 5.0, -0.0), 0.0) and same(fma(-0.0, 5.0, -0.0), -0.0)
    assert same(fma(1.5, 2.0, -3.0), 0.0) and same(fma(-1.5, 2.0, 3.0), 0.0)              # x + (-x) = +0
    assert same(fma(0.0, 5.0, 7.0), 7.0) and same(fma(2.0, 0.0, -den), -den)
    # the rounding to fp32 the oracle applies
    d32 = 2.0 ** -149
    with np.errstate(over="ignore"):
        assert np.float32(0.75 * d32) == np.float32(d32) and np.float32(1.5 * d32) == np.float32(2 * d32)
        z = np.float32(-0.25 * d32)
        assert z == 0 and np.signbit(z) and np.isinf(np.float32(4.0 * float(np.finfo(np.float32).max)))
    # the edge pools hold what their docstring says, exactly, and the oracle carries them
    for kind, t in (("x64", np.float64), ("x32", np.float32)):
        a = tf.pool(kind)
        fi = np.finfo(t)
        assert a.dtype == t and a.shape == (tf.POOL, tf.LMAX) and np.isfinite(a).all()
        sub = (a != 0) & (np.abs(a) < fi.tiny)
        assert sub.any() and np.signbit(a[a == 0]).any() and not np.signbit(a[a == 0]).all()
        assert (a == fi.max).any() and (a == -fi.max).any() and (np.abs(a) == fi.smallest_subnormal).any()
        for p in range(tf.POOL):
            at = np.flatnonzero(np.abs(a[p]) == fi.max)
            assert at.size >= 8 and np.diff(at).min() >= 20
    w4 = np.array([4.0, -4.0, 4.0, -4.0, 4.0])
    got = tf.oracle("x32", 0, w4, 300, True)
    assert got.dtype == np.float32 and np.isposinf(got).any() and np.isneginf(got).any() and not np.isnan(got).any()
    wide = tf.oracle("x32", 0, w4, 300, False)
    assert np.isfinite(wide).all() and np.abs(wide).max() == 4.0 * float(np.finfo(np.float32).max)
    half = np.array([0.25, -0.5, 0.25])
    for kind, out32, t in (("x64", False, np.float64), ("x32", True, np.float32)):
        got = tf.oracle(kind, 1, half, 400, out32)
        tiny = np.finfo(t).tiny
        assert ((got != 0) & (np.abs(got) < tiny)).any() and np.signbit(got[got == 0]).any()
    # the random pools: the plain chain, as before
    w = tf.weights(5, 1)[0]
    for kind, out32 in (("f64", False), ("f32", True), ("f32", False)):
        row = [Fr(float(v)) for v in tf.pool(kind)[2]]
        want = []
        for t in range(20):
            acc = 0.0
            for k in range(5):
                acc = float(Fr(float(w[k])) * row[t + k] + Fr(acc))
            want.append(np.float32(acc) if out32 else acc)
        want = np.array(want, dtype=np.float32 if out32 else np.float64)
        assert np.array_equal(tf.bits(tf.oracle(kind, 2, w, 20, out32)), tf.bits(want))


# ---- front-end refusals before the device -------------------------------------------------------------------------------
def _tiny(nt=12):
    la = -90 + (np.arange(6) + 0.5) * 30.0
    lat = np.repeat(la, 8)
    lon = np.tile(np.arange(8) * 45.0, 6)
    plev = np.array([100.0, 500.0, 1000.0])
    return lat, lon, plev, np.zeros((lat.size, 3, nt))


W3 = [0.25, 0.5, 0.25]
BAD = [
    (dict(time_bands=[W3]), "mapping"),
    (dict(time_bands={}), "1..4 bands"),
    (dict(time_bands={str(i): W3 for i in range(5)}), "1..4 bands"),
    (dict(time_bands={"": W3}), "non-empty strings"),
    (dict(time_bands={3: W3}), "non-empty strings"),
    (dict(time_bands={"a": [0.5, 0.5]}), "odd"),
    (dict(time_bands={"a": [1.0]}), "odd and in 3..255"),
    (dict(time_bands={"a": np.ones(257)}), "odd and in 3..255"),
    (dict(time_bands={"a": np.ones((3, 3))}), "one-dimensional"),
    (dict(time_bands={"a": [0.25, np.nan, 0.25]}), "finite"),
    (dict(time_bands={"a": [0.25, np.inf, 0.25]}), "finite"),
    (dict(time_bands={"a": ["x", "y", "z"]}), "sequence of numbers"),
    (dict(time_bands={"a": W3, "b": np.ones(13) / 13}), "NT >= 2h \\+ 1 = 13"),
    (dict(time_bands={"a": W3}, time_block=4), "time_block="),
    (dict(time_bands={"a": W3}, missing="mask"), "missing='mask'"),
    (dict(time_bands={"a": W3}, climatology=True), "climatology=True"),
    (dict(time_bands={"a": W3}, wavenumbers=(1,), lon="ok"), "wavenumbers="),
]


@pytest.mark.parametrize("kw,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_time_bands_are_refused_before_device(kw, match):
    from pytemdiags_amd import TEMDiagnostics
    lat, lon, plev, f = _tiny()
    kw = dict(kw)
    if "lon" in kw:
        kw["lon"] = lon
    with pytest.raises(ValueError, match=match):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, L=10, device=99, **kw)
    with pytest.raises(ValueError, match=match):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=plev, ps=np.zeros((lat.size, 12)), hyam=np.zeros(3),
                                         hybm=np.ones(3), L=10, device=99, **kw)


def test_time_bands_keyword_is_keyword_only_and_off_by_default():
    from pytemdiags_amd import TEMDiagnostics, climatology, timebands
    p = inspect.signature(TEMDiagnostics.__init__).parameters["time_bands"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert isinstance(TEMDiagnostics.bands, property)
    names, table, h = timebands.check_bands({"s": [1.0, -2.0, 1.0], "l": np.arange(7.0)})
    assert names == ("s", "l") and h == 3 and table.shape == (2, 7) and table.dtype == np.float64
    assert np.array_equal(table[0], [0, 0, 1, -2, 1, 0, 0]) and np.array_equal(table[1], np.arange(7.0))   # padded, centred
    assert timebands.check_record((names, table, h), 7)[2] == 3
    with pytest.raises(ValueError, match="NT >= 2h"):
        timebands.check_record((names, table, h), 6)
    assert timebands.clim is climatology and timebands.NB_MAX == 4 and (timebands.NW_MIN, timebands.NW_MAX) == (3, 255)


# ---- Lanczos weights -----------------------------------------------------------------------------------------------------
def _duchon(nw, fc):
    """Duchon (1979), eq. for the low-pass weights, scaled to unit sum."""
    n = (nw - 1) // 2
    k = np.arange(-n, n + 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.sin(2 * np.pi * fc * k) / (np.pi * k) * np.sinc(k / n)
    w[n] = 2 * fc
    return w / w.sum()


def _response(w, f):
    n = (w.size - 1) // 2
    return float(np.sum(w * np.cos(2 * np.pi * f * np.arange(-n, n + 1))))


@pytest.mark.parametrize("nw", [3, 9, 31, 121, 255])
def test_lanczos_weights(nw):
    from pytemdiags_amd.timebands import lanczos
    lo, hi, bp = lanczos(nw, low=0.2), lanczos(nw, high=0.1), lanczos(nw, low=0.25, high=0.125)
    for w, total in ((lo, 1.0), (hi, 0.0), (bp, 0.0)):
        assert w.shape == (nw,) and w.dtype == np.float64 and np.array_equal(w, w[::-1])
        assert abs(math.fsum(w) - total) <= 1e-15, (nw, math.fsum(w))
    n = (nw - 1) // 2
    delta = np.zeros(nw)
    delta[n] = 1.0
    assert np.max(np.abs(lo - _duchon(nw, 0.2))) <= 1e-15
    assert np.max(np.abs(hi - (delta - _duchon(nw, 0.1)))) <= 1e-15
    assert np.max(np.abs(bp - (_duchon(nw, 0.25) - _duchon(nw, 0.125)))) <= 1e-15
    if nw == 121:
        assert abs(_response(lo, 0.2) - 0.5) <= 0.02 and abs(_response(hi, 0.1) - 0.5) <= 0.02
        assert abs(_response(bp, 0.25) - 0.5) <= 0.02 and abs(_response(bp, 0.125) - 0.5) <= 0.02
        assert abs(_response(lo, 0.05) - 1.0) <= 0.01 and abs(_response(lo, 0.4)) <= 0.01
        assert abs(_response(bp, 0.19) - 1.0) <= 0.01 and abs(_response(bp, 0.03)) <= 0.01 and abs(_response(bp, 0.4)) <= 0.01


def test_lanczos_refusals():
    from pytemdiags_amd.timebands import lanczos
    for args, kw in (((8,), dict(low=0.2)), ((1,), dict(low=0.2)), ((257,), dict(low=0.2)), ((9.0,), dict(low=0.2)),
                     ((9,), dict()), ((9,), dict(low=0.5)), ((9,), dict(high=0.0)), ((9,), dict(low=0.1, high=0.2))):
        with pytest.raises(ValueError):
            lanczos(*args, **kw)
