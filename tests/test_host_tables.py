"""The host code that decides what every sweep reads and how every launch is cut -- class_tables.hpp, side_tables.hpp,
host_math.hpp and launch_shapes.hpp of pytemdiags_amd/csrc, none of which needs HIP -- run on its own through
tests/host/host_tables_main.cpp.  The program is built twice with g++, plain and with AddressSanitizer + UBSan, and
every case runs under both: (a) invariants of the tables, (b) equality with the tables recorded before the code moved
out of temx.hip (tests/golden/host_tables.json), (c) the numerics against numpy, (d) the launch shapes."""
import hashlib
import itertools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytemdiags_amd", "csrc")
HOST_HEADERS = ("shared_defs.hpp", "side_tables.hpp", "class_tables.hpp", "host_math.hpp", "launch_shapes.hpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_tables.json")

CLS_MB, CLS_PADB, CLS_HASPAD_BIT, CLS_SOUTH, CLS_FIRST, CLS_LAST = 4, 10, 1 << 27, 1, 2, 4     # shared_defs.hpp
PAD = -2 ** 31
TOL64, TOL32 = 1e-11, 1e-8                     # degrees: fp64 plans, fp32 plans (TEMX_LAT_TOL_F32)
CUT = {"f64": (TOL64, 0, 0), "f32": (TOL32, 8, 16)}      # tolerance, TEMX_F32_SIDE_CAP, TEMX_F32_SIDE_KEEP
NSUBS = (1, 2, 7, 64)
KEEP = 4                                       # class-groups the subsample keeps (the library: 32)

SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
_PROGRAMS = {}


def programs(tmp_path_factory):
    """{"plain": path, "asan": path}, built once per session (test_vertical_host.py shares them)."""
    if not _PROGRAMS:
        if shutil.which("g++") is None:
            pytest.skip("no g++")
        d = tmp_path_factory.mktemp("host_tables")
        src = os.path.join(ROOT, "tests", "host", "host_tables_main.cpp")
        jobs = {}
        for name, extra in (("plain", []), ("asan", SANITIZE)):
            exe = str(d / ("host_tables_" + name))
            jobs[name] = (exe, subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, src, "-o", exe,
                                                 "-pthread"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        for name, (exe, p) in jobs.items():
            out = p.communicate()[0]
            assert p.returncode == 0, out
            _PROGRAMS[name] = exe
        _PROGRAMS["dir"] = str(d)
        _PROGRAMS["count"] = 0
    return _PROGRAMS


def runner(build, tmp_path_factory):
    """run(command, input array or None, numbers ...) -> {name: array} of what the program wrote."""
    progs = programs(tmp_path_factory)
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


@pytest.fixture(params=["plain", "asan"])
def run(request, tmp_path_factory):
    return runner(request.param, tmp_path_factory)


# ---- grids ---------------------------------------------------------------------------------------------------------
def _rows(rows, nlon):
    return np.repeat(np.asarray(rows, dtype=np.float64), nlon)


def grid(name):
    from pytemdiags_amd import synth
    if name.startswith("ne"):
        return synth.cubed_sphere_gll(int(name[2:]))[0]
    if name == "handoff":          # test_gpu_sweep_handoff.py: 40 mirrored pairs of rows and an equator row, 4 longitudes
        north = (np.arange(40) + 0.5) * (90.0 / 40.5)
        return _rows(np.concatenate([-north[::-1], [0.0], north]), 4)
    if name == "latlon":           # 64 rows x 1440 longitudes and 33 more columns on the equator
        north = (np.arange(32) + 0.5) * (90.0 / 32.5)
        return np.concatenate([_rows(np.concatenate([-north[::-1], north]), 1440), np.zeros(33)])
    if name == "hemisphere":       # 12 rows x 9, all northern: classes with an empty southern side
        return _rows((np.arange(12) + 0.5) * 7.0, 9)
    if name == "equator":          # one class of 100
        return np.zeros(100)
    raise KeyError(name)


GRIDS = ("ne2", "ne4", "ne8", "handoff", "latlon", "hemisphere", "equator")
SYMMETRIC = ("ne2", "ne4", "ne8", "handoff", "latlon", "equator")


def refused():
    rng = np.random.default_rng(3)
    bad = np.tile(np.linspace(-80.0, 80.0, 9), 9)
    nan, over = bad.copy(), bad.copy()
    nan[40] = np.nan
    over[40] = 91.0
    return {"distinct": rng.uniform(-89.0, 89.0, 500), "n63": np.repeat(np.linspace(-60.0, 60.0, 7), 9), "nan": nan,
            "over": over}


def tables(run, lat, mode, L=0, nstripes=1):
    """The class tables of `lat` with everything derived from them; cuts for NSUBS and for one piece more than there
    are class-groups."""
    tol, cap, keep_side = CUT[mode]
    t = run("classes", lat, tol, cap, keep_side, KEEP, L, nstripes, *NSUBS)
    if t["ok"][0]:
        more = run("classes", lat, tol, cap, keep_side, KEEP, 0, 1, int(t["dims"][1]) + 1)
        t.update({k: v for k, v in more.items() if "cut_" in k})
    return t


# ---- (a) invariants ------------------------------------------------------------------------------------------------
def _batches(crow, nbatch):
    c = crow.reshape(-1, 4, CLS_MB)
    assert c.shape[0] == nbatch + CLS_PADB and np.all(c[nbatch:] == PAD)        # the tail the index loads run into
    real = c[:nbatch]
    return real, real < 0, real & 0x07FFFFFF, (real >> 28) & 7, (real >> 27) & 1


def _check_flags(flag, gb0, ngroups):
    """Per group: northern batches, then southern; FIRST on the first batch only, LAST on the last only."""
    first = np.zeros(flag.size, bool)
    last = np.zeros(flag.size, bool)
    first[gb0[:-1]] = True
    last[gb0[1:] - 1] = True
    assert np.array_equal((flag & CLS_FIRST) != 0, first) and np.array_equal((flag & CLS_LAST) != 0, last)
    south = (flag & CLS_SOUTH).astype(np.int64)
    inner = np.ones(flag.size, bool)
    inner[gb0[:-1]] = False
    assert np.all(np.diff(south)[inner[1:]] >= 0)


def check_class_tables(lat, t, mode):
    tol = CUT[mode][0]
    N = lat.size
    ncls, ngroups, nbatch, max_side = (int(x) for x in t["dims"])
    gb0 = t["gbatch0"].astype(np.int64)
    assert ngroups == (ncls + 3) // 4 and gb0.size == ngroups + 1
    assert gb0[0] == 0 and gb0[-1] == nbatch and np.all(np.diff(gb0) >= 1)
    real, pad, rows, flags, haspad = _batches(t["crow"], nbatch)
    assert np.array_equal(np.sort(rows[~pad]), np.arange(N))                    # every column exactly once
    assert np.all(flags == flags[:, :1, :1]) and np.all(haspad == haspad[:, :1, :1])
    assert np.array_equal(haspad[:, 0, 0] != 0, pad.any(axis=(1, 2)))
    assert np.all(rows[pad] == 0)
    bflag = flags[:, 0, 0]
    _check_flags(bflag, gb0, ngroups)
    grp = np.repeat(np.arange(ngroups), np.diff(gb0))
    side = bflag & CLS_SOUTH
    # members per (group, side, slot), their |lat| and hemisphere
    g3 = np.broadcast_to(grp[:, None, None], rows.shape)
    s3 = np.broadcast_to(side[:, None, None], rows.shape)
    k3 = np.broadcast_to(np.arange(4)[None, :, None], rows.shape)
    idx = (g3[~pad], s3[~pad], k3[~pad])
    la = lat[rows[~pad]]
    counted = np.zeros((ngroups, 2, 4))
    np.add.at(counted, idx, 1.0)
    assert np.array_equal(counted, t["cnt"].reshape(ngroups, 2, 4))
    assert max_side == int(counted.max())
    nb_side = np.stack([np.bincount(grp[side == s], minlength=ngroups) for s in (0, 1)], axis=1)
    assert np.array_equal(nb_side, np.ceil(counted / CLS_MB).max(axis=2).astype(np.int64))
    assert np.all(la[idx[1] == 0] >= -tol) and np.all(la[idx[1] == 1] < -tol)
    lo = np.full((ngroups, 4), np.inf)
    hi = np.full((ngroups, 4), -np.inf)
    tot = np.zeros((ngroups, 4))
    np.minimum.at(lo, (idx[0], idx[2]), np.abs(la))
    np.maximum.at(hi, (idx[0], idx[2]), np.abs(la))
    np.add.at(tot, (idx[0], idx[2]), np.abs(la) - lo[idx[0], idx[2]])
    n = counted.sum(axis=1)
    used = n > 0
    assert int(used.sum()) == ncls and np.all(used.ravel()[:ncls])
    assert np.all((hi - lo)[used] <= tol)
    mean = lo[used] + tot[used] / n[used]
    xc = t["xc"].reshape(ngroups + 1, 4)
    assert np.max(np.abs(xc[:ngroups][used] - np.cos(np.deg2rad(90.0 - mean)))) <= 1e-14
    assert np.all(xc[:ngroups][~used] == 0.0) and np.all(xc[ngroups] == 0.0)
    return dict(ncls=ncls, ngroups=ngroups, nbatch=nbatch, max_side=max_side, gb0=gb0, real=real, pad=pad, rows=rows,
                side=side, counted=counted)


def check_side_tables(t, c, pre=""):
    gb0 = (t[pre + "gbatch0"] if pre else t["gbatch0"]).astype(np.int64)
    ngroups = gb0.size - 1
    crow = t[pre + "crow"].reshape(-1, 4 * CLS_MB)[:gb0[-1]]
    south = ((crow[:, 0] >> 28) & CLS_SOUTH) != 0
    for sd in (0, 1):
        gf = t["%sside%d_gfirst" % (pre, sd)].astype(np.int64)
        assert gf.size == ngroups + 1 and gf[0] == 0 and np.all(np.diff(gf) >= 1)
        sc = t["%sside%d_crow" % (pre, sd)].reshape(-1, 4 * CLS_MB)
        assert sc.shape[0] == gf[-1] + CLS_PADB and np.all(sc[gf[-1]:] == PAD)
        sc = sc[:gf[-1]]
        _check_flags((sc[:, 0] >> 28) & 7 & ~CLS_SOUTH, gf, ngroups)
        assert np.all(((sc >> 28) & 7) == ((sc[:, :1] >> 28) & 7))
        mine = np.flatnonzero(south == bool(sd))
        per_group = np.bincount(np.repeat(np.arange(ngroups), np.diff(gb0))[mine], minlength=ngroups)
        assert np.array_equal(np.diff(gf), np.maximum(per_group, 1))
        empty = np.repeat(per_group == 0, np.diff(gf))
        assert np.all(sc[empty] == (PAD | ((CLS_FIRST | CLS_LAST) << 28) | CLS_HASPAD_BIT))
        keep = ~(7 << 28)                               # rows, padding sign and has-padding bit, in the same order
        assert np.array_equal(sc[~empty] & keep, crow[mine] & keep)


def check_cuts(t, gb0, nbatch, ngroups, pre=""):
    for nsub in (*NSUBS, ngroups + 1):
        for kind in ("aligned",) if pre else ("aligned", "plain"):
            key = "%scut_%s_%d" % (pre, kind, nsub)
            if key not in t:
                assert pre and nsub == ngroups + 1       # (the extra piece count is that of the full table)
                continue
            cut = t[key].reshape(nsub + 1, 2).astype(np.int64)
            b, g = cut[:, 0], cut[:, 1]
            assert tuple(cut[0]) == (0, 0) and b[-1] == nbatch and np.all(np.diff(b) >= 0) and np.all(np.diff(g) >= 0)
            if kind == "aligned":
                assert g[-1] == ngroups and np.array_equal(b, gb0[g])
            else:       # a plain cut names the group its batch lies in; the end of the list belongs to the last group
                assert np.all(g < ngroups) and np.all(gb0[g] <= b)
                assert np.all((b < gb0[g + 1]) | (b == nbatch)) and g[-1] == ngroups - 1


def check_subsample(t, c):
    S, sg, sb = (int(x) for x in t["sub_dims"])
    assert S == max(1, min(256, c["ngroups"] // KEEP))
    groups = np.arange(0, c["ngroups"], S)
    assert sg == groups.size
    gb0 = c["gb0"]
    sgb0 = t["sub_gbatch0"].astype(np.int64)
    assert np.array_equal(np.diff(sgb0), (gb0[groups + 1] - gb0[groups])) and sgb0[0] == 0 and sgb0[-1] == sb
    full = t["crow"].reshape(-1, 4 * CLS_MB)
    want = np.concatenate([full[gb0[g]:gb0[g + 1]] for g in groups] + [np.full((CLS_PADB, 4 * CLS_MB), PAD, np.int32)])
    assert t["sub_crow"].tobytes() == want.astype("<i4").tobytes()
    assert np.array_equal(t["sub_xc"], np.concatenate([t["xc"].reshape(-1, 4)[groups].ravel(), np.zeros(4)]))
    check_side_tables(t, c, "sub_")
    check_cuts(t, sgb0, sb, sg, "sub_")


# the issue's figures for these grids: (classes, groups, longest side)
EXPECT = {("ne4", "f64"): (64, 16, 48), ("ne4", "f32"): (69, 18, 8), ("handoff", "f64"): (41, 11, 4),
          ("equator", "f32"): (13, 4, 8), ("ne8", "f64"): (246, 62, None), ("ne2", "f64"): (None, None, 24)}


@pytest.mark.parametrize("name", GRIDS)
def test_class_tables_hold_their_invariants(run, name):
    lat = grid(name)
    classes = {}
    for mode in ("f64", "f32"):
        t = tables(run, lat, mode)
        assert t["ok"][0] == 1
        c = check_class_tables(lat, t, mode)
        print(name, mode, {k: c[k] for k in ("ncls", "ngroups", "nbatch", "max_side")})
        for got, want in zip((c["ncls"], c["ngroups"], c["max_side"]), EXPECT.get((name, mode), (None,) * 3)):
            assert want is None or got == want
        check_side_tables(t, c)
        check_cuts(t, c["gb0"], c["nbatch"], c["ngroups"])
        check_subsample(t, c)
        # the classes as (northern rows, southern rows)
        members = {}
        grp = np.repeat(np.arange(c["ngroups"]), np.diff(c["gb0"]))
        for b, k, j in zip(*np.nonzero(~c["pad"])):
            members.setdefault((grp[b], k), ([], []))[c["side"][b]].append(int(c["rows"][b, k, j]))
        classes[mode] = {(tuple(n), tuple(s)) for n, s in members.values()}
        classes[mode + "_t"] = t
    # the fp32 cut: no side above 16, and a class with a side above 8 is one the cut left alone
    assert max(max(len(n), len(s)) for n, s in classes["f32"]) <= 16
    assert all((n, s) in classes["f64"] for n, s in classes["f32"] if max(len(n), len(s)) > 8)
    if name == "ne2":
        assert max(max(len(n), len(s)) for n, s in classes["f32"]) <= 8
    if name == "ne8":                                   # no long side: the same table, bit for bit
        assert all(classes["f64_t"][k].tobytes() == classes["f32_t"][k].tobytes() for k in classes["f64_t"])
    if name == "equator":
        assert classes["f64_t"]["dims"].tolist() == [1, 1, 25, 100]
    if name == "latlon":
        assert lat.size == 92193 and classes["f64_t"]["dims"][3] == 1440 and classes["f32_t"]["dims"][3] == 8


@pytest.mark.parametrize("name", ["distinct", "n63", "nan", "over"])
def test_grids_without_usable_classes_are_refused(run, name):
    lat = refused()[name]
    assert lat.size == {"distinct": 500, "n63": 63, "nan": 81, "over": 81}[name]
    for mode in ("f64", "f32"):
        assert run("classes", lat, *CUT[mode], KEEP, 0, 1)["ok"][0] == 0
    if name in ("nan", "over"):
        assert run("mirror", lat, TOL64)["ok"][0] == 0


@pytest.mark.parametrize("name", SYMMETRIC)
def test_mirror_pairs(run, name):
    lat = grid(name)
    for tol in (TOL64, TOL32):
        m = run("mirror", lat, tol)
        assert m["ok"][0] == 1
        n, s = m["rowN"].astype(np.int64), m["rowS"].astype(np.int64)
        assert np.array_equal(np.sort(np.concatenate([n, s[s >= 0]])), np.arange(lat.size))
        assert np.all(np.diff(n) > 0)
        eq = np.abs(lat[n]) <= tol
        assert np.array_equal(s < 0, eq)
        assert np.all(lat[n[~eq]] > tol) and np.all(np.abs(lat[n[~eq]] + lat[s[~eq]]) <= tol)
    drop = int(np.argmax(np.abs(lat) > 1.0)) if name != "equator" else None
    if drop is not None:
        assert run("mirror", np.delete(lat, drop), TOL64)["ok"][0] == 0


def test_one_hemisphere_has_no_mirror_pairs(run):
    assert run("mirror", grid("hemisphere"), TOL64)["ok"][0] == 0


# ---- (b) pinned against the tables recorded before the code moved --------------------------------------------------
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<i4").tobytes()).hexdigest()


def split_cases(run):
    """choose_split arguments of temx_plan_set_tem (and more) for ne4 x 30 x 2 and ne30 x 72 x 91 on 256 CUs."""
    from pytemdiags_amd import synth
    rows = []
    for ne, D in ((4, 60), (30, 6552)):
        lat = synth.cubed_sphere_gll(ne)[0]
        t = run("classes", lat, TOL64, 0, 0, 32, 0, 1)
        _, cgroups, cbatches, _ = (int(x) for x in t["dims"])
        sbatches = int(t["sub_dims"][2])
        nchunk, cu, cunits = (lat.size + 15) // 16, 256, max(1, cbatches // 4)
        rows += [(D, nchunk, 2 * cu, 4, 4), (D, max(1, cunits // 4), cu, 1, 8), (D, max(1, sbatches // 4), cu, 4, 2),
                 (D, max(1, cgroups // 8), cu, 1, 1)]
        rows += [(D, nchunk, w * cu, d, 4) for w in (2, 3) for d in (1, 4)]
        rows += [(D, cunits, w * cu, d, m) for w in (1, 2, 3) for d in (1, 4) for m in (1, 8)]
        for e in (1, 2, 4):
            rows += [(D, nchunk // (8 // e), cu, e, 4), (D, cunits // (8 // e), cu, e, 1), (D, max(1, cgroups // (8 // e)), cu, e, 1)]
    return np.array(rows, dtype=np.float64)


def vert_cases():
    from test_vertical_host import SWEEP, TIE_CASES
    rows = [(nf, nlev, nt, nplev, np.dtype(dt).itemsize, 0 if pmode == "hybrid" else np.dtype(pdt).itemsize)
            for nf, nlev, nt, nplev, dt, pmode, pdt, _, _ in SWEEP]
    rows += [(nf, nlev, nt, {26: 11, 13: 9}[nlev], 8, 0 if pmode == "hybrid" else 8) for nlev, nt, pmode, nf, _ in TIE_CASES]
    return np.array(rows, dtype=np.float64)


def layout_cases():
    """The shapes of test_gpu_layout.py: (ncol, nlev, ntb, bytes per destination element)."""
    rows = list(itertools.product((1, 37, 64, 866, 1025), (1, 2, 9), (1, 7, 33, 70), (4, 8)))
    rows += [(ncol, nlev, ntb, dsz) for ntb, dsz in ((130, 8), (300, 8), (300, 4), (64, 8), (128, 4))
             for ncol, nlev in ((37, 2), (130, 3))]
    rows += [(6, 4, 50, 4), (6, 4, 48, 8), (1048579, 8, 4, 4), (1048579, 8, 65, 8)]
    return np.array(rows, dtype=np.float64)


INT_TABLES = ("crow", "gbatch0", "side0_crow", "side0_gfirst", "side1_crow", "side1_gfirst", "sub_crow", "sub_gbatch0",
              "sub_side0_crow", "sub_side0_gfirst", "sub_side1_crow", "sub_side1_gfirst")


def pinned_records(run):
    """What tests/golden/host_tables.json holds: SHA-256 of the integer tables, the small double arrays themselves."""
    ints, dbls = {}, {}
    for name in GRIDS:
        for mode in ("f64", "f32"):
            t = tables(run, grid(name), mode)
            for k in sorted(t):
                if k in INT_TABLES or "cut_" in k or k in ("dims", "sub_dims"):
                    ints["%s/%s/%s" % (name, mode, k)] = _sha(t[k])
    for name in refused():
        ints["%s/ok" % name] = _sha(run("classes", refused()[name], *CUT["f32"], KEEP, 0, 1)["ok"])
    for name in SYMMETRIC:
        m = run("mirror", grid(name), TOL64)
        ints["%s/mirror" % name] = _sha(np.concatenate([m["rowN"], m["rowS"]]))
    ints["split"] = _sha(run("split", split_cases(run))["split"])
    ints["vert"] = _sha(run("vert", vert_cases())["vert"])
    ints["layout"] = _sha(run("layout", layout_cases())["layout"])
    t = tables(run, grid("ne4"), "f64", L=12, nstripes=3)
    for k in ("xc", "cnt", "Gs", "Gx"):
        dbls["ne4/" + k] = t[k].tolist()
    q = run("quad", None, 26, 25)                      # L = 12: 2L + 2 nodes, degrees to 2L
    dbls["L12/Yq"], dbls["L12/w2"] = q["Y"].tolist(), q["w2"].tolist()
    return {"sha256": ints, "float64": dbls}


def test_tables_equal_those_recorded_before_the_move(run):
    want = json.load(open(GOLDEN))
    got = pinned_records(run)
    assert got["sha256"].keys() == want["sha256"].keys() and got["float64"].keys() == want["float64"].keys()
    for k, h in want["sha256"].items():
        assert got["sha256"][k] == h, k
    for k, v in want["float64"].items():
        a, b = np.array(got["float64"][k]), np.array(v)
        assert a.shape == b.shape and np.all(np.abs(a - b) <= 1e-14 * np.abs(b)), k


# ---- (c) numerics against numpy -----------------------------------------------------------------------------------
# Every bound is ten times the error measured with the plain build (given next to it), and never looser than 1e-12.
def _ylm0(x, n):
    """Y_l^0(x), l < n, from numpy's Legendre polynomials."""
    from numpy.polynomial import legendre
    return np.stack([np.sqrt((2 * l + 1) / (4 * np.pi)) * legendre.legval(x, [0] * l + [1]) for l in range(n)], axis=-1)


def _gram(lat, K):
    y = _ylm0(np.cos(np.deg2rad(90.0 - lat)), K)
    return y.T @ y


def test_gauss_legendre_matches_numpy(run):
    from numpy.polynomial.legendre import leggauss
    for n, bound in ((2, 2.2e-15), (3, 1.1e-15), (26, 3.9e-15), (102, 2.6e-14)):     # measured 0 (bound: ten ulp), 1.1e-16, 3.9e-16, 2.6e-15
        q = run("quad", None, n, 1)
        x, w = leggauss(n)
        err = max(np.max(np.abs(q["x"] - x)), np.max(np.abs(q["w"] - w)))
        print("gauss_legendre(%d): %.1e" % (n, err))
        assert err <= bound


def test_ylm0_is_orthonormal_under_the_quadrature(run):
    q = run("quad", None, 102, 51)
    Y = q["Y"].reshape(102, 51)
    assert np.array_equal(q["w2"], q["w2"][::-1]) or np.max(np.abs(q["w2"] - q["w2"][::-1])) <= 1e-16
    err = np.max(np.abs((Y * q["w2"][:, None]).T @ Y - np.eye(51)))
    print("orthonormality to degree 50: %.1e" % err)
    assert err <= 5.6e-15                                                    # measured 5.6e-16
    err = np.max(np.abs(Y - _ylm0(q["x"], 51)))
    print("ylm0_row against numpy's legval: %.1e" % err)
    assert err <= 8.2e-13                                                    # measured 8.2e-14 (legval's own recurrence at degree 50)


def test_gradient_table_matches_numpy_gradient(run):
    rng = np.random.default_rng(0)
    cases = {"uniform": np.arange(40) * 0.125 + 3.0, "nonuniform": np.sort(rng.uniform(0.0, 10.0, 37)),
             "pressure": np.exp(np.linspace(np.log(100.0), np.log(1e5), 30)), "n2": np.array([1.0, 2.5]),
             "n3": np.array([1.0, 2.5, 3.0]), "n3u": np.array([1.0, 2.0, 3.0])}
    for name, x in cases.items():
        tab = run("gradient", x)["tab"].reshape(-1, 3)
        f = rng.standard_normal(x.size)
        got = tab[:, 1] * f
        got[1:] += tab[1:, 0] * f[:-1]
        got[:-1] += tab[:-1, 2] * f[1:]
        want = np.gradient(f, x, edge_order=1)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print("gradient_table %s: %.1e" % (name, err))
        assert err <= 1.3e-15                                                # measured <= 1.3e-16
        assert tab[0, 0] == 0.0 and tab[-1, 2] == 0.0


def test_spd_inverse_of_the_gram_matrix(run):
    from pytemdiags_amd import synth
    lat = synth.cubed_sphere_gll(4)[0]
    for K, bound in ((13, 2.1e-15), (51, 1.4e-16)):   # measured |G Ginv - I| / cond(G): 2.1e-16, 1.4e-17
        G = _gram(lat, K)
        r = run("spd", G, K)
        assert r["rc"][0] == 0
        err = np.max(np.abs(G @ r["Ginv"].reshape(K, K) - np.eye(K))) / np.linalg.cond(G)
        print("spd K = %d: cond %.1e, |G Ginv - I| / cond = %.1e" % (K, np.linalg.cond(G), err))
        assert err <= bound
        assert np.array_equal(r["Ginv"].reshape(K, K), r["Ginv"].reshape(K, K).T)
    bad = _gram(lat, 13)
    bad[5, 5] = -1.0
    assert run("spd", bad, 13)["rc"][0] == -1
    bad = _gram(lat, 13)
    bad[3, 2] = bad[2, 3] = np.nan
    assert run("spd", bad, 13)["rc"][0] == -1
    assert run("spd", _gram(np.repeat(np.linspace(-60.0, 60.0, 5), 20), 8), 8)["rc"][0] == -1    # rank 5 < 8


def test_sym_pinv_of_a_rank_deficient_gram_matrix(run):
    G = _gram(np.repeat(np.array([-61.0, -23.0, 4.0, 37.0, 70.0]), 20), 8)
    r = run("pinv", G, 8)
    assert r["rc"].tolist() == [0, 5]
    want = np.linalg.pinv(G, hermitian=True)
    w = np.linalg.eigvalsh(G)
    cond = w[-1] / w[3]                                # over the five eigenvalues that count
    err = np.max(np.abs(r["Ginv"].reshape(8, 8) - want)) / np.max(np.abs(want)) / cond
    print("sym_pinv: cond %.1e, relative difference / cond = %.1e" % (cond, err))
    assert err <= 2.1e-15                                                    # measured 2.1e-16


def test_block_packers_recover_the_matrix(run):
    rng = np.random.default_rng(1)
    for R, K, TB in ((7, 5, 2), (13, 13, 4), (4, 3, 1), (50, 51, 13)):
        A = rng.standard_normal((R, K))
        blk = run("blocks4", A, R, K, TB)["blk"].reshape((R + 3) // 4, TB, 4, 4)     # [rb][t][k][i]
        full = blk.transpose(0, 3, 1, 2).reshape(4 * ((R + 3) // 4), 4 * TB)
        want = np.zeros_like(full)
        want[:R, :K] = A
        assert np.array_equal(full, want)
    for R, C, ld, tr, nrb4, nkb in ((13, 13, 13, 0, 4, 4), (13, 13, 13, 1, 4, 4), (26, 13, 25, 0, 8, 4), (13, 26, 25, 1, 4, 8),
                                    (5, 3, 7, 0, 2, 1), (3, 5, 7, 1, 5, 2), (13, 10, 13, 0, 4, 4)):
        A = rng.standard_normal((C if tr else R, ld))
        out = run("blocks16", A, R, C, ld, tr, nrb4, nkb)["blk"]
        assert np.array_equal(out[:3], [-1.0] * 3)         # appended behind what was there
        nrb = (nrb4 + 3) // 4
        blk = out[3:].reshape(nrb, nkb, 4, 16)             # [rb][t][k][m]
        full = blk.transpose(0, 3, 1, 2).reshape(16 * nrb, 4 * nkb)
        want = np.zeros_like(full)
        want[:R, :C] = (A[:C, :R].T if tr else A[:R, :C])
        assert np.array_equal(full, want)


def test_tem_tables_match_numpy(run):
    from pytemdiags_amd import synth
    p = synth.pressure_levels(30) * 100.0
    lat = np.linspace(-88.5, 88.5, 60)
    t = run("tem", np.concatenate([p, lat]), 30, 3, 101325.0)
    assert np.array_equal(t["pg"], run("gradient", p)["tab"]) and np.array_equal(t["lg"], run("gradient", np.deg2rad(lat))["tab"])
    assert np.max(np.abs(t["coslat"] - np.cos(lat * np.pi / 180.0))) <= 1e-15
    assert np.max(np.abs(t["fcor"] - 2 * 7.29212e-5 * np.sin(lat * np.pi / 180.0))) <= 1e-19
    want = np.repeat((101325.0 / p) ** (287.058 / 1004.64), 3)
    assert np.max(np.abs(t["colscale"] / want - 1.0)) <= 1e-15


def test_missing_value_tables_match_numpy(run):
    """miss_tables: G2 | Zq = Y(x_q) T | Yq = 2 pi w_q Y(x_q) | Acov = Gi T^T | c1 = Gi T^T Y0^T 1."""
    from numpy.polynomial.legendre import leggauss
    from pytemdiags_amd import synth
    L, K = 6, 7
    x = np.cos(np.deg2rad(90.0 - synth.cubed_sphere_gll(2)[0]))
    rng = np.random.default_rng(2)
    T = np.triu(rng.standard_normal((K, K))) + 3.0 * np.eye(K)
    G2, Gi = rng.standard_normal((K, K)), rng.standard_normal((K, K))
    tab = run("miss", np.concatenate([G2.ravel(), T.ravel(), Gi.ravel(), x]), K, L)["mtab"]
    NQ = NE = 2 * L + 1
    xq, wq = leggauss(NQ)
    Y = _ylm0(xq, NE)
    want = np.concatenate([G2.ravel(), (Y[:, :K] @ T).ravel(), (2 * np.pi * wq[:, None] * Y).ravel(), (Gi @ T.T).ravel(),
                           Gi @ T.T @ _ylm0(x, K).sum(axis=0)])
    assert tab.size == want.size
    err = np.max(np.abs(tab - want)) / np.max(np.abs(want))
    print("miss_tables: %.1e" % err)
    assert err <= 2.5e-14                                                    # measured 2.5e-15


# ---- (d) launch shapes ---------------------------------------------------------------------------------------------
def test_layout_tile_covers_the_window_within_the_lds_tile(run):
    cases = layout_cases()
    out = run("layout", cases)["layout"].reshape(-1, 7)
    seen = set()
    for (ncol, nlev, ntb, dsz), (tc_shift, kl, tt, stride, nct, nlt, ntt) in zip(cases.astype(np.int64), out.astype(np.int64)):
        assert tc_shift in (5, 6) and kl >= 1 and tt >= 1
        assert (kl * tt << tc_shift) * dsz <= 32 * 1024                      # the tile
        assert stride % 2 == 1 and kl * tt <= stride <= kl * tt + 1
        assert (stride << tc_shift) * dsz <= 33 * 1024                       # LAYOUT_LDS_BYTES, with the padding
        assert (nct << tc_shift) >= ncol > ((nct - 1) << tc_shift)
        assert nlt * kl >= nlev > (nlt - 1) * kl and ntt * tt >= ntb > (ntt - 1) * tt
        assert tt == ntb or kl == 1
        seen.add((int(tc_shift), kl > 1, ntt > 1))
    assert seen == {(6, True, False), (6, False, False), (5, False, False), (6, False, True)}


def test_choose_split_fills_the_slots(run):
    cases = split_cases(run)
    out = run("split", cases)["split"].reshape(-1, 4)
    for (D, nchunk, slots, dpw, minchunk), (ndt, nsplit, grid_, dpw_out) in zip(cases.astype(np.int64), out.astype(np.int64)):
        assert ndt == (D + 15) // 16 and dpw_out == dpw
        assert 1 <= nsplit <= max(1, nchunk // minchunk) and nsplit <= 4096
        nwg = -(-ndt // dpw) * nsplit
        assert grid_ % 8 == 0 and nwg <= grid_ < nwg + 8


def test_choose_split_of_the_masked_tracer_shapes(run):
    """The cuts test_gpu_masked_tracer_variants.py relies on, as launch_miss_tracer_project asks for them on 256 CUs
    (slots = 2 * 256, four d-tiles per workgroup): cs8 has 217 chunks.  D = 1300 must keep ranges of at least 9 chunks
    (whole groups on the clamp-free path of miss_tracer_project_kernel: three at a ring two deep), D = 21 the ranges of
    4 or 5 of the small cases, and three chunks are one range."""
    cases = np.array([(1300, 217, 512, 4, 4), (21, 217, 512, 4, 4), (3, 3, 512, 4, 4)], dtype=np.float64)
    out = run("split", cases)["split"].reshape(-1, 4).astype(np.int64)
    assert out[:, 0].tolist() == [82, 2, 1] and out[:, 3].tolist() == [4, 4, 4]
    assert out[:, 1].tolist() == [24, 54, 1]
    nchunk, nsplit = 217, int(out[0, 1])
    ranges = [nchunk * (s + 1) // nsplit - nchunk * s // nsplit for s in range(nsplit)]
    assert sum(ranges) == nchunk and min(ranges) >= 9
