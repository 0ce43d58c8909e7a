"""What temx_plan_set_tem decides (pytemdiags_amd/csrc/tem_layout.hpp): the form of the latitude-class sweeps, the cut of
every launch and the size of every buffer, as pure functions -- on their own, plain and under AddressSanitizer + UBSan
(tests/host/tem_layout_main.cpp).  Needs no GPU.

(a) tests/golden/tem_layouts.json holds what the library decided before this logic left temx.hip, recorded on an MI355X
    by tools/record_tem_layouts.py: per temx_plan_set_tem call every input, the buffers and cuts the plan held before
    (b_*) and after (a_*).  The header must give every one of them again.
(b) synthetic cases around each threshold, and every environment override against every option value.
(c) invariants over all of them.
"""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tem_layouts.json")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
BUFFERS = ("B4", "B3", "C4", "zb", "Bs", "csum", "pbuf", "Pq", "Ax", "Axs", "osAt", "osAb", "rho", "rho0")
SPLITS = ("proj4", "eddy", "proj1", "cproj4", "cproj1", "ceddy", "cflux", "lflux", "copw", "os", "os_s", "sproj4", "sproj1",
          "seddy")
LDS_BYTES = 163840            # of a compute unit
_PROGRAMS = {}


def programs(tmp_path_factory):
    if not _PROGRAMS:
        if shutil.which("g++") is None:
            pytest.skip("no g++")
        d = tmp_path_factory.mktemp("tem_layout")
        src = os.path.join(ROOT, "tests", "host", "tem_layout_main.cpp")
        jobs = {}
        for name, extra in (("plain", []), ("asan", SANITIZE)):
            exe = str(d / ("tem_layout_" + name))
            jobs[name] = (exe, subprocess.Popen(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, src, "-o", exe],
                                                stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        for name, (exe, p) in jobs.items():
            out = p.communicate()[0]
            assert p.returncode == 0, out
            _PROGRAMS[name] = exe
        _PROGRAMS["dir"], _PROGRAMS["count"] = str(d), 0
    return _PROGRAMS


def _value(v):
    return [int(x) for x in v.split(",")] if "," in v else (int(v) if v.lstrip("-").isdigit() else v)


@pytest.fixture(params=["plain", "asan"])
def run(request, tmp_path_factory):
    """run(command, cases) -> one {key: value} per case, as the program printed it."""
    progs = programs(tmp_path_factory)
    if request.param == "asan" and os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")

    def run(cmd, cases=None):
        args = [progs[request.param], cmd]
        if cases is not None:
            progs["count"] += 1
            path = os.path.join(progs["dir"], "in%d.txt" % progs["count"])
            with open(path, "w") as fh:
                for c in cases:
                    fh.write(" ".join("%s=%s" % (k, ",".join(map(str, v)) if isinstance(v, list) else v) for k, v in c.items()) + "\n")
            args.append(path)
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (cmd, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        rows = [{k: _value(v) for k, v in (tok.split("=", 1) for tok in line.split())} for line in r.stdout.splitlines()]
        assert cases is None or len(rows) == len(cases)
        return rows
    return run


def recorded():
    doc = json.load(open(GOLDEN))
    assert doc["count"] == len(doc["records"])
    return doc["records"]


def asks(out):
    a = out["partial_asks"]
    return a if isinstance(a, list) else [a]


def expected_after(v, out):
    """The plan after the call: a buffer grows to what it is asked to hold and never shrinks, a cut is the one assigned
    or stays."""
    exp = {"a_partial": max([v["b_partial"]] + asks(out))}
    for b in BUFFERS:
        exp["a_" + b] = max(v["b_" + b], out.get("need_" + b, 0))
    for s in SPLITS:
        exp["a_sp_" + s] = out.get("sp_" + s, v["b_sp_" + s])
    for flag in ("onepass", "lone", "os_on"):
        exp[flag] = out[flag]
    return exp


# ---- (a) -----------------------------------------------------------------------------------------------------------------
def test_every_recorded_call_is_decided_as_before_the_move(run):
    recs = recorded()
    outs = run("plan", [r["v"] for r in recs])
    assert len(recs) >= 40
    for r, out in zip(recs, outs):
        v = r["v"]
        exp = expected_after(v, out)
        assert len(exp) == 1 + len(BUFFERS) + len(SPLITS) + 3
        got = {k: v[k] for k in exp}
        assert got == exp, (r["name"], {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]})
        # the memory rule was asked, and the tables of the single sweep were built, exactly where the header says
        assert (v["os_rc"] != -1000) == bool(out["want_os"]), r["name"]
        assert v["os_rc"] in (-1000, 0, -4), r["name"]


def test_the_recorded_calls_take_every_branch():
    vs = {r["name"]: r["v"] for r in recorded()}
    seen = lambda pred: any(pred(v) for v in vs.values())
    D = lambda v: v["nlev"] * v["nt"]
    assert seen(lambda v: v["cls"] and not v["onepass"]) and seen(lambda v: v["onepass"] and not v["os_on"])
    assert seen(lambda v: v["os_on"])        # (no recorded grid has too few latitudes for the reference fit: TEMX_ERANK is synthetic)
    assert seen(lambda v: v["lcls"] and v["lone"]) and seen(lambda v: v["lcls"] and not v["lone"] and D(v) < 49)
    assert seen(lambda v: v["lcls"] and not v["lone"] and D(v) >= 49)                   # held to two passes by the option
    assert seen(lambda v: v["sym"] and not v["cls"]) and seen(lambda v: not (v["sym"] or v["cls"] or v["lcls"]))
    assert seen(lambda v: v["weighted"] and v["unfused"]) and seen(lambda v: v["bin"]) and seen(lambda v: v["TBS"] == 8)
    # csum held from an earlier call: too small (the rule is asked again, free > 0) and large enough (it is not)
    for path in ("cls", "lcls"):
        assert seen(lambda v: v[path] and 0 < v["b_csum"] < v["a_csum"] and v["free"] > 0)
        assert seen(lambda v: v[path] and (v["onepass"] or v["lone"]) and v["b_csum"] == v["a_csum"] > 0)
    assert seen(lambda v: v["cls"] and v["onepass"] and v["b_csum"] > 0 and v["free"] == 0)
    assert {v["opt_form"] for v in vs.values()} == {-1, 0, 1, 2, 3}
    assert {v["L"] for v in vs.values()} >= {20, 50, 60, 70} and {D(v) for v in vs.values()} >= {21, 60, 2160, 240, 248}
    assert {v["N"] for v in vs.values()} == {866, 3458, 48602, 92193}
    for key in ("env_two_pass", "env_one_pass", "env_single_sweep"):
        assert seen(lambda v: v[key] != "-")
    groups = vs["ne30_L50_above/0"]["cgroups"]
    assert groups > 640 and {v["min_groups"] for v in vs.values() if v["N"] == 48602} >= {-1, 700, 800} and 700 < groups < 800
    assert vs["ne30_L50_below/0"]["N"] * 240 < 1.2e7 <= vs["ne30_L50_above/0"]["N"] * 248
    assert not vs["ne30_L50_below/0"]["onepass"] and vs["ne30_L50_above/0"]["os_on"]


# ---- (b) -----------------------------------------------------------------------------------------------------------------
def base_case(name, **kw):
    """A recorded call on a fresh plan with nothing held and plenty of memory, then changed."""
    v = dict(next(r["v"] for r in recorded() if r["name"] == name))
    for k in v:
        if k.startswith("b_") and not k.startswith("b_sp_"):
            v[k] = 0
    v.update(free=1 << 40, os_rc=0)
    v.update(kw)
    return v


def test_the_memory_rule_of_the_class_sums(run):
    """Held already, or less than half of what is free: free at 2 need and 2 need + 1 refuses, 2 need + 2 grants."""
    need = run("plan", [base_case("ne30_L50_above/0")])[0]["need_csum"]
    frees = (2 * need - 2, 2 * need, 2 * need + 1, 2 * need + 2, 4 * need)
    outs = run("plan", [base_case("ne30_L50_above/0", free=f) for f in frees])
    assert [o["onepass"] for o in outs] == [0, 0, 0, 1, 1] and all(o["want_onepass"] for o in outs)
    assert all("need_csum" not in o and "sp_cflux" not in o and o["os_on"] == 0 for o in outs[:3])
    # held: no free memory is needed; one byte short of held is not held
    outs = run("plan", [base_case("ne30_L50_above/0", free=0, b_csum=h) for h in (need, need + 512, need - 1, 0)])
    assert [o["onepass"] for o in outs] == [1, 1, 0, 0]


def test_the_memory_rule_of_the_large_L_class_sums(run):
    """Both streams together in less than half of what is free, unless csum is held."""
    o = run("plan", [base_case("ne8_L70_long/0")])[0]
    assert o["lone"] == 1
    both = o["need_csum"] + o["need_pbuf"]
    outs = run("plan", [base_case("ne8_L70_long/0", free=f) for f in (2 * both - 2, 2 * both, 2 * both + 1, 2 * both + 2,
                                                                      2 * o["need_csum"] + 2)])
    assert [x["lone"] for x in outs] == [0, 0, 0, 1, 0]
    outs = run("plan", [base_case("ne8_L70_long/0", free=0, b_csum=h) for h in (o["need_csum"], o["need_csum"] - 1)])
    assert [x["lone"] for x in outs] == [1, 0]


def test_the_group_count_that_takes_the_single_sweep(run):
    outs = run("plan", [base_case("ne30_L50_above/0", cgroups=g, min_groups=m)
                        for g, m in ((639, -1), (640, -1), (640, 641), (639, 639), (5, 0))])
    assert [o["want_os"] for o in outs] == [0, 1, 0, 1, 1] and [o["os_on"] for o in outs] == [0, 1, 0, 1, 1]
    assert all(o["onepass"] for o in outs)
    # TEMX_ERANK from the tables: wanted, not taken
    o = run("plan", [base_case("ne30_L50_above/0", os_rc=-4)])[0]
    assert (o["want_os"], o["os_on"], o["onepass"]) == (1, 0, 1) and "sp_os" not in o


@pytest.mark.parametrize("nlev,nt,n_at", [(2, 32, 187500), (7, 7, 244898)])
def test_the_size_that_takes_the_one_pass_form(run, nlev, nt, n_at):
    """1.2e7 elements per field: the first column count at or above it, and the one below."""
    D = nlev * nt
    assert (n_at - 1) * D < 1.2e7 <= n_at * D
    outs = run("plan", [base_case("ne30_L50_above/0", nlev=nlev, nt=nt, N=n) for n in (n_at - 1, n_at)])
    assert [o["want_onepass"] for o in outs] == [0, 1] and [o["onepass"] for o in outs] == [0, 1]
    # fewer than four d-tiles: never, whatever the size and the option
    o = run("plan", [base_case("ne30_L50_above/0", nlev=2, nt=24, N=1 << 30, opt_form=1)])[0]
    assert o["want_onepass"] == 0


def test_every_environment_override_against_every_option(run):
    """The environment wins over temx_plan_configure; TEMX_ONE_PASS can only add; latitude bins ignore both."""
    option = {-1: (0, 0, -1), 0: (1, 0, 0), 1: (0, 1, 0), 2: (0, 1, 1), 3: (0, 0, 0)}
    envs = ("-", "0", "1", "x")
    cases = [dict(opt_form=f, bin=b, env_two_pass=t, env_one_pass=o, env_single_sweep=s)
             for f in option for b in (0, 1) for t in envs for o in envs for s in envs]
    outs = run("form", cases)
    assert len(outs) == 5 * 2 * 64
    for c, got in zip(cases, outs):
        two, force, os_ = option[c["opt_form"]]
        if c["env_two_pass"] != "-":
            two = int(c["env_two_pass"] == "1")
        force = int(force or c["env_one_pass"] == "1")
        os_ = {"0": 0, "1": 1}.get(c["env_single_sweep"], os_)
        exp = (1, 0, 0) if c["bin"] else (two, force, os_)
        assert (got["two_pass"], got["force_op"], got["os"]) == exp, c


# ---- (c) -----------------------------------------------------------------------------------------------------------------
def synthetic_cases():
    rows = []
    for name in ("ne30_L50_above/0", "ne8_L70_long/0", "ne8_sym_L50_long/0", "ne8_generic_L20_lev/0", "latlon_L20_small/0"):
        for nlev, nt in ((2, 1), (7, 3), (3, 16), (2, 32), (9, 9), (72, 91), (128, 1000)):
            for form, cu in itertools.product((-1, 0, 1, 2), (256, 304, 8)):
                rows.append(base_case(name, nlev=nlev, nt=nt, opt_form=form, num_cu=cu))
    return rows


def check_splits(v, out):
    """What test_host_tables.py::test_choose_split_fills_the_slots asserts, with the work units and the smallest piece of
    every cut written out."""
    D = v["nlev"] * v["nt"]
    ndt, e = (D + 15) // 16, out["edpw"]
    cunits, nch = max(1, v["cbatches"] // 4), (v["npg"] + 2) // 3
    one = out["onepass"]
    units = {"proj4": (v["nchunk"], 4, 1 if e == 1 else 4), "eddy": (v["nchunk"] // (8 // e), 4, e), "proj1": (v["nchunk"], 4, 4),
             "cproj4": (cunits, 8, 4) if one or out["lone"] else (cunits, 1, 4 if e == 4 else 1), "cproj1": (cunits, 1, 4),
             "ceddy": (cunits // (8 // e), 1, e), "cflux": (max(1, v["cgroups"] // (8 // e)), 1, e),
             "lflux": (max(1, v["cgroups"] // 8), 1, 1), "copw": (max(1, cunits // 4), 8, 1), "os": (cunits, 8, 4),
             "os_s": (max(1, v["sbatches"] // 4), 2, 4), "sproj4": (nch, 4, 4 if e == 4 else 1), "sproj1": (nch, 4, 4),
             "seddy": (v["npg"] // (8 // e), 4, e)}
    assert e in (1, 2, 4) and -(-ndt // e) * e <= 1.05 * max(-(-ndt // 4) * 4, ndt) + e
    for s in SPLITS:
        if "sp_" + s not in out:
            continue
        ndt_out, nsplit, grid_, dpw = out["sp_" + s]
        if s == "sproj1" and e != 4:
            assert (ndt_out, nsplit, grid_, dpw) == (0, 0, 0, 4)          # not used: one field per wave
            continue
        nchunk, minchunk, dpw_exp = units[s]
        assert ndt_out == ndt and dpw == dpw_exp, s
        assert 1 <= nsplit <= max(1, nchunk // minchunk) and nsplit <= 4096, s
        nwg = -(-ndt // dpw) * nsplit
        assert grid_ % 8 == 0 and nwg <= grid_ < nwg + 8, s


def test_invariants_of_every_layout(run):
    cases = [r["v"] for r in recorded()] + synthetic_cases()
    outs = run("plan", cases)
    for v, out in zip(cases, outs):
        KD8 = v["K"] * v["nlev"] * v["nt"] * 8
        assert max([v["b_partial"]] + asks(out)) >= max(asks(out)) > 0
        assert out["tracer_Bq"] == KD8 and out["tracer_partial"] % KD8 == 0
        # the tracer's projection fits what the TEM sweeps asked for (their cuts are at least as fine)
        assert out["tracer_partial"] <= max(asks(out))
        assert out["os_on"] <= out["onepass"] <= out["want_onepass"] and out["os_on"] <= out["want_os"]
        assert not (out["lone"] and out["onepass"])
        for b in BUFFERS:
            assert out.get("need_" + b, 8) % 8 == 0
        check_splits(v, out)


def test_lds_of_the_single_sweep_kernels(run):
    """Every instantiation the launcher makes fits the LDS of a compute unit: the three (TBS, TBX) pairs of dispatch.hpp,
    the kinds 0, 1 and 3 of kernels_op2.hpp, the library's TEMX_OS_DEFER = 1.  sweep_os_kernel (the tile map) is never
    built for kind 3 -- launch_sweep_os_t refuses two tracers per sweep there -- and would not fit at (7, 13)."""
    rows = run("lds")
    assert len(rows) == 3 * 3 * 2 and {(r["TBS"], r["TBX"]) for r in rows} == {(7, 13), (4, 8), (2, 4)}
    for r in rows:
        assert r["os2"] <= LDS_BYTES and r["osr"] <= LDS_BYTES, r
        if r["kind"] != 3:
            assert r["os"] <= LDS_BYTES, r
        assert r["os"] % 8 == 0 and r["os2"] % 8 == 0 and r["osr"] % 8 == 0
    worst = next(r for r in rows if (r["TBS"], r["kind"], r["DF"]) == (7, 0, 1))
    assert (worst["os"], worst["os2"], worst["osr"]) == (145408, 154240, 154256)     # as temx.hip computed them inline
