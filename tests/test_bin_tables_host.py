"""The host tables of the latitude-bin sweeps -- pytemdiags_amd/csrc/bin_tables.hpp, which needs no HIP -- run on their
own through tests/host/bin_tables_main.cpp.  The program is built twice with g++, plain and with AddressSanitizer +
UBSan, and every case runs under both: (a) invariants of the sorted rows and chunks, (b) the choice of the Chebyshev
degree J, (c) the interpolated basis rows against the oracle's recurrence, (d) the front end's argument checks (no device).

The rule for J is the one of include/temx.h: the smallest of {8, 10, 12} with 2 (L h / 2)^J / J! <= 1e-13, h = pi / (2 B).
By that rule (50, 128) gets J = 12 (bound 2.9e-15) and (63, 256) gets J = 10 (bound 4.0e-14): neither is refused, and the
interpolated rows at both are checked to 1e-12 below like every served pair.  What the rule refuses needs a degree beyond
the library's L <= 63, e.g. (100, 128)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import tem_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_PROGRAMS = {}


def programs(tmp_path_factory):
    if not _PROGRAMS:
        if shutil.which("g++") is None:
            pytest.skip("no g++")
        d = tmp_path_factory.mktemp("bin_tables")
        src = os.path.join(ROOT, "tests", "host", "bin_tables_main.cpp")
        jobs = {}
        for name, extra in (("plain", []), ("asan", SANITIZE)):
            exe = str(d / ("bin_tables_" + name))
            jobs[name] = (exe, subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, src, "-o", exe],
                                                stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        for name, (exe, p) in jobs.items():
            out = p.communicate()[0]
            assert p.returncode == 0, out
            _PROGRAMS[name] = exe
        _PROGRAMS["dir"] = str(d)
        _PROGRAMS["count"] = 0
    return _PROGRAMS


@pytest.fixture(params=["plain", "asan"])
def run(request, tmp_path_factory):
    progs = programs(tmp_path_factory)
    build = request.param
    if build == "asan" and os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")

    def run(cmd, arr, *nums):
        progs["count"] += 1
        base = os.path.join(progs["dir"], "io%d" % progs["count"])
        inp = "-"
        if arr is not None:
            inp = base + ".in"
            np.ascontiguousarray(arr, dtype="<f8").tofile(inp)
        r = subprocess.run([progs[build], cmd, inp, base + ".out", *[repr(float(x)) for x in nums]], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, (cmd, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        raw = open(base + ".out", "rb").read()
        out, o = {}, 0
        while o < len(raw):
            nl = int(np.frombuffer(raw, "<i4", 1, o)[0])
            name = raw[o + 4:o + 4 + nl].decode()
            kind = int(np.frombuffer(raw, "<i4", 1, o + 4 + nl)[0])
            n = int(np.frombuffer(raw, "<i8", 1, o + 8 + nl)[0])
            dt = "<f8" if kind else "<i4"
            out[name] = np.frombuffer(raw, dt, n, o + 16 + nl).copy()
            o += 16 + nl + n * np.dtype(dt).itemsize
        for f in (inp, base + ".out"):
            if f != "-":
                os.remove(f)
        return out
    return run


# ---- grids ---------------------------------------------------------------------------------------------------------
def edges(B):
    """edge(i) = -pi/2 + i (pi / B), the expression of bin_tables.hpp"""
    return -0.5 * np.pi + np.arange(B + 1) * (np.pi / B)


def crowded(B=512, seed=5):
    """2000 columns: 900 inside [30.00, 30.05] degrees, two at exactly +-90, one on each of ten inner bin edges, the
    rest random (a fifth of the bins stays empty at B = 512)."""
    rng = np.random.default_rng(seed)
    on_edges = np.rad2deg(edges(B)[1:-1][np.linspace(3, B - 5, 10).astype(int)])
    rest = np.rad2deg(np.arcsin(rng.uniform(-1, 1, 2000 - 900 - 2 - 10)))
    lat = np.concatenate([rng.uniform(30.0, 30.05, 900), [90.0, -90.0], on_edges, rest])
    return lat[rng.permutation(lat.size)]


def grid(name, B):
    rng = np.random.default_rng(3)
    if name == "random":
        return np.rad2deg(np.arcsin(rng.uniform(-1, 1, 3000)))
    if name == "crowded":
        return crowded(B)
    if name == "one-latitude":
        return np.full(1300, 12.3456)
    if name == "single":
        return np.array([-41.0])
    if name == "poles":
        return np.array([90.0, -90.0, 90.0, -90.0, 90.0])
    if name == "edges":
        return np.rad2deg(edges(B)[1:-1])
    raise KeyError(name)


GRIDS = ("random", "crowded", "one-latitude", "single", "poles", "edges")


def numpy_bins(lat, B):
    """A column on an inner edge belongs to the upper bin, +pi/2 to the last."""
    return np.searchsorted(edges(B)[1:-1], lat * (np.pi / 180.0), side="right")


# ---- (a) rows and chunks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [128, 512])
@pytest.mark.parametrize("name", GRIDS)
def test_rows_and_chunks(run, name, B):
    lat = grid(name, B)
    t = run("rows", lat, B)
    assert t["ok"][0] == 1
    R = int(t["ok"][1])
    assert 1 <= R <= 4096
    n = lat.size
    rows, s, chunk, c0 = t["rows"], t["s"], t["chunk"].reshape(-1, 4), t["bin_chunk0"]
    want = numpy_bins(lat, B)
    # a stable sort by bin
    assert np.array_equal(rows, np.argsort(want, kind="stable"))
    assert np.all(np.abs(s) <= 1.0)
    h = np.pi / (2 * B)
    centre = -0.5 * np.pi + (want[rows] + 0.5) * (np.pi / B)
    assert np.allclose(s, np.clip((lat[rows] * (np.pi / 180.0) - centre) / h, -1, 1), rtol=0, atol=1e-12)
    # every row in exactly one chunk; chunks never span bins, hold 1..R rows and come in sorted order
    seen = np.zeros(n, dtype=int)
    pos = 0
    for b, first, cnt, pad in chunk:
        assert first == pos and 1 <= cnt <= R and pad == 0
        assert np.all(want[rows[first:first + cnt]] == b)
        seen[rows[first:first + cnt]] += 1
        pos += cnt
    assert pos == n and np.all(seen == 1)
    assert np.all(np.diff(chunk[:, 0]) >= 0)
    # only the last chunk of a bin may be short
    for i in range(len(chunk) - 1):
        if chunk[i, 0] == chunk[i + 1, 0]:
            assert chunk[i, 2] == R
    # first chunk of every bin; empty bins have none
    assert c0.size == B + 1 and c0[0] == 0 and c0[-1] == len(chunk)
    counts = np.bincount(want, minlength=B)
    assert np.array_equal(np.diff(c0), -(-counts // R))
    if name == "crowded":
        assert np.max(np.diff(c0)) >= 2 or R >= 900
        if B == 512:
            assert np.count_nonzero(counts == 0) >= 50          # empty bins have no chunk
    if name == "edges":                      # a latitude on edge i belongs to bin i (a few move by the rounding of
        assert np.count_nonzero(want == np.arange(1, B)) >= (B - 1) // 2     # the conversion to degrees and back)
    if name == "poles":
        assert set(want) == {0, B - 1} and np.all(np.abs(np.abs(s) - 1.0) < 1e-12)


def test_rows_refuse_bad_latitudes(run):
    for bad in (np.array([0.0, np.nan]), np.array([0.0, 90.5]), np.array([-91.0])):
        assert run("rows", bad, 128)["ok"][0] == 0


# ---- (b) the degree ------------------------------------------------------------------------------------------------
def rule(L, B):
    h = np.pi / (2 * B)
    for J in (8, 10, 12):
        if 2.0 * (L * h / 2) ** J / math.factorial(J) <= 1e-13:
            return J
    return 0


def test_degree_rule(run):
    pairs = [(20, 128), (50, 512), (63, 512), (63, 2048), (50, 256), (50, 128), (63, 256), (63, 128), (100, 128), (200, 256)]
    t = run("degree", None, *[x for p in pairs for x in p])
    J = t["J"].reshape(-1, 2)
    for (L, B), (j, ok) in zip(pairs, J):
        assert j == rule(L, B), (L, B, j)
        assert ok == 1
    got = dict(zip(pairs, J[:, 0]))
    assert got[(20, 128)] == 10 and got[(50, 512)] == 8 and got[(63, 512)] == 10 and got[(63, 2048)] == 8
    assert got[(50, 256)] == 10
    # see the module docstring: the rule serves these two, with the largest / the middle degree
    assert got[(50, 128)] == 12 and got[(63, 256)] == 10
    # refused: no J of the set meets the bound
    assert got[(100, 128)] == 0 and got[(200, 256)] == 0
    bound = t["bound"].reshape(-1, 3)
    assert abs(bound[1, 0] / 6e-14 - 1) < 0.1          # (50, 512, 8): the 6e-14 of the formulation
    bad = run("degree", None, 50, 100, 50, 0, 50, 4096)["J"].reshape(-1, 2)
    assert np.all(bad[:, 1] == 0)                      # bin counts outside the allowed set


# ---- (c) the tables ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B", [(20, 128), (50, 512), (63, 512), (63, 2048), (50, 128), (63, 256)])
def test_interpolated_rows_match_the_recurrence(run, L, B):
    rng = np.random.default_rng(11)
    lat = np.concatenate([np.rad2deg(rng.uniform(-np.pi / 2, np.pi / 2, 9990)), [90.0, -90.0, 0.0],
                          np.rad2deg(edges(B)[[1, B // 2, B - 1]]), [89.9999, -89.9999, 30.0, 1e-9]])
    assert lat.size == 10000
    t = run("basis", lat, L, B)
    assert t["J"][0] == rule(L, B)
    Y = t["Y"].reshape(lat.size, L + 1)
    ref = orc.ylm0_matrix_recurrence(lat, L)
    e = float(np.max(np.abs(Y - ref)))
    print("(L, B, J) = (%d, %d, %d): max |interpolant - Y_l| = %.2e" % (L, B, t["J"][0], e))
    assert e <= 1e-12, e
    # the tables depend on (L, B, J) only and are zero beyond l = L
    a = t["a"].reshape(B, t["J"][0], t["J"][1])
    assert np.all(a[:, :, L + 1:] == 0.0) and np.all(np.isfinite(a))


def test_refused_pair_has_no_tables(run):
    assert run("basis", np.array([0.0]), 100, 128)["J"][0] == 0


# ---- (d) the front end, without a device ---------------------------------------------------------------------------
def test_lat_bins_values():
    from pytemdiags_amd import _lib, engine
    assert (_lib.OPT_LAT_BINS, _lib.OPT_BIN_DEGREE, _lib.FORM_BINNED) == (12, 13, 5)
    assert engine.lat_bins_value(None) == 0 and engine.lat_bins_value(False) == 0 and engine.lat_bins_value(0) == 0
    assert engine.lat_bins_value(True) == -1
    for b in (128, 256, 512, 1024, 2048):
        assert engine.lat_bins_value(b) == b
    for bad in (100, -1, 1, 4096, 512.0, "512", [512]):
        with pytest.raises(ValueError):
            engine.lat_bins_value(bad)


def test_header_declares_the_options():
    text = open(os.path.join(ROOT, "include", "temx.h")).read()
    for decl in ("TEMX_OPT_LAT_BINS = 12", "TEMX_OPT_BIN_DEGREE = 13", "TEMX_FORM_BINNED = 5"):
        assert decl in text, decl


def test_lat_bins_with_mask_raises_before_the_device():
    from pytemdiags_amd import TEMDiagnostics, sph_zonal_averager
    lat = np.linspace(-80, 80, 50)
    x = np.zeros((50, 3, 2))
    with pytest.raises(ValueError, match="lat_bins"):
        TEMDiagnostics(x, x, x, x, lat, plev=np.array([100.0, 500.0, 900.0]), missing="mask", lat_bins=True, device=99)
    with pytest.raises(ValueError, match="lat_bins"):
        TEMDiagnostics(x, x, x, x, lat, plev=np.array([100.0, 500.0, 900.0]), lat_bins=100, device=99)
    with pytest.raises(ValueError, match="lat_bins"):
        sph_zonal_averager(lat, np.arange(-90.0, 91.0), 10, missing="mask", lat_bins=512, device=99)
    with pytest.raises(ValueError, match="lat_bins"):
        sph_zonal_averager(lat, np.arange(-90.0, 91.0), 10, lat_bins=100, device=99)
    with pytest.raises(ValueError, match="lat_bins"):
        TEMDiagnostics.from_model_levels(x, x, x, x, lat, plev=np.array([500.0]), ps=np.zeros((50, 2)),
                                         hyam=np.zeros(3), hybm=np.ones(3), missing="mask", lat_bins=True, device=99)
