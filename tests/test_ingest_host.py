"""Time-major model-level records, host side: the ctypes table against include/temx_ingest.h, the plain-C link check,
the argument checks that must fail before any device call, the tile chooser against its numpy mirror (the library's
code built stand-alone with AddressSanitizer + UBSan), the front end's refusals and the gate.  Needs no GPU."""
import itertools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_vertical_host import hybrid_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TM = ("time", "lev", "ncol")


# ---- header, bindings, plain-C consumer ---------------------------------------------------------------------------
def test_ingest_header_declares_exactly_what_is_bound():
    import ctypes as C
    from pytemdiags_amd import _ingest, _lib
    hdr = open(os.path.join(ROOT, "include", "temx_ingest.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(temxi_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _ingest.SIGNATURES} == {"temxi_version", "temxi_records_to_pressure"}
    assert not re.findall(r"\b(temx[vl]?_[a-z0-9_]+)\s*\(", code)   # the other headers' ABI is not extended from here
    assert '#include "temx.h"' in code
    lib = _ingest.load()
    assert lib is _lib.load() and lib.temxi_version() == _ingest.INGEST_VERSION == 100
    assert re.search(r"\bTEMXI_NF_MAX = %d\b" % _ingest.NF_MAX, code) and _ingest.NF_MAX == 8
    # the declared parameter list, type by type, against the argtypes
    decl = re.search(r"int temxi_records_to_pressure\((.*?)\);", code, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "void*": C.c_void_p, "const void*": C.c_void_p,
             "const void* const*": C.POINTER(C.c_void_p), "void* const*": C.POINTER(C.c_void_p),
             "const int*": C.POINTER(C.c_int), "const double*": C.POINTER(C.c_double)}
    want = [ctype[p.rsplit(" ", 1)[0]] for p in params]
    sig = dict((n, (r, a)) for n, r, a in _ingest.SIGNATURES)
    assert sig["temxi_records_to_pressure"] == (C.c_int, want)
    assert sig["temxi_version"] == (C.c_int, [])
    assert [p.rsplit(" ", 1)[1] for p in params] == [
        "device", "nf", "src_host", "src_dtype_host", "dst_host", "dst_dtype", "ncol", "nlev", "nt_src", "t0", "ntb",
        "nplev", "plev_pa_host", "hyam_host", "hybm_host", "p0_hybrid", "ps", "ps_dtype", "method", "edge", "stream"]
    # the entry point with a body is a function-try-block, like every other one; the other three versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    assert re.search(r"^int temxi_records_to_pressure\([^;{]*\)\s*try \{\s*$", src, re.M)
    assert "int temxi_version(void) { return 100; }" in src
    assert "int temx_version(void) { return 402; }" in src and "int temxv_version(void) { return 100; }" in src
    assert "int temxl_version(void) { return 100; }" in src


def test_ingest_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_ingest")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_ingest.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxi_version=100 nf_max=8 nf0_rc=-1" in out.stdout


def test_ingest_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _ingest
    lib = _ingest.load()
    plev = (C.c_double * 2)(5e4, 7e4)
    hy = (C.c_double * 3)(0.1, 0.2, 0.3)
    src, dst = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(1 << 20)
    f64, f32 = (C.c_int * 1)(0), (C.c_int * 1)(1)
    ps0 = C.c_void_p(1 << 24)

    def call(nf=1, src=src, sdt=f64, dst=dst, ddt=0, ncol=4, nlev=3, nt_src=5, t0=1, ntb=2, nplev=2, plev=plev, hyam=hy,
             hybm=hy, p0=1e5, ps=ps0, pdt=0, method=0, edge=0):
        # device 99 does not exist: a call that got as far as the device would come back TEMX_EHIP, not TEMX_EINVAL
        return lib.temxi_records_to_pressure(99, nf, src, sdt, dst, ddt, ncol, nlev, nt_src, t0, ntb, nplev, plev, hyam,
                                             hybm, p0, ps, pdt, method, edge, None)

    def refused(word=None, **kw):
        rc = call(**kw)
        msg = lib.temx_last_error()
        assert rc == -1 and msg, (kw, rc, msg)
        if word is not None:
            assert word in msg, (kw, msg)
    refused(b"nf", nf=0)
    refused(b"nf", nf=9)
    for name in ("src", "sdt", "dst", "plev", "hyam", "hybm", "ps"):
        refused(b"null", **{name: None})
    refused(b"null", src=(C.c_void_p * 1)(None))
    refused(b"null", dst=(C.c_void_p * 1)(None))
    refused(nlev=1)
    refused(ncol=0)
    refused(ntb=0)
    refused(nplev=0)
    refused(nt_src=0)
    refused(b"t0", t0=-1)
    refused(b"nt_src", t0=4)                                       # t0 + ntb = 6 > nt_src = 5
    refused(b"nt_src", ntb=6, t0=0)
    refused(b"plev", plev=(C.c_double * 2)(7e4, 5e4))              # not ascending
    refused(b"plev", plev=(C.c_double * 2)(5e4, 5e4))
    refused(b"plev", plev=(C.c_double * 2)(-1.0, 5e4))
    refused(b"plev", plev=(C.c_double * 2)(5e4, float("inf")))
    refused(b"finite", hyam=(C.c_double * 3)(0.1, float("nan"), 0.3))
    refused(b"finite", hybm=(C.c_double * 3)(0.1, 0.2, float("inf")))
    refused(b"finite", p0=float("nan"))
    refused(ddt=2)
    refused(pdt=2)
    refused(sdt=(C.c_int * 1)(7))
    refused(b"method", method=2)
    refused(b"edge", edge=-1)
    refused(b"narrow", sdt=f64, ddt=1)                             # fp64 -> fp32
    refused(b"aligned", src=(C.c_void_p * 1)(4096 + 4))
    refused(b"aligned", dst=(C.c_void_p * 1)((1 << 20) + 4))
    refused(b"aligned", ps=C.c_void_p((1 << 24) + 2), pdt=1)
    refused(b"overlaps", dst=src)
    refused(b"overlaps", dst=(C.c_void_p * 1)(4096 + 64))          # partial overlap is aliasing too
    refused(b"overlaps ps", dst=(C.c_void_p * 1)((1 << 24) + 8))
    two_src = (C.c_void_p * 2)(4096, 8192)
    two_f64 = (C.c_int * 2)(0, 0)
    refused(b"overlaps dst", nf=2, src=two_src, sdt=two_f64, dst=(C.c_void_p * 2)(1 << 20, (1 << 20) + 16))
    # well-formed: only now is the device touched
    assert call() == -2
    assert call(sdt=f32, ddt=1, pdt=1, method=1, edge=1) == -2
    assert call(nf=2, src=two_src, sdt=two_f64, dst=(C.c_void_p * 2)(1 << 20, 1 << 21)) == -2
    assert call(nlev=2, plev=(C.c_double * 1)(5e4), nplev=1, hyam=(C.c_double * 2)(0.1, 0.2),
                hybm=(C.c_double * 2)(0.0, 0.5)) == -2


# ---- the tile chooser ------------------------------------------------------------------------------------------------
THREADS, LDS_BYTES = 256, 48 * 1024                                # shared_defs.hpp: INGEST_THREADS, INGEST_LDS_BYTES


def ingest_tile(ncol, nlev, ntb, nf, dsz, ssz):
    """Host mirror of ingest_tile (launch_shapes.hpp): TT = 128 bytes of destination or the whole window, halved until
    two level slots fit; TC = 128 bytes of the narrowest source, doubled while the tile has no pair for every lane;
    KW = the level slots the budget holds, less one.  None: no tile."""
    if ncol < 1 or nlev < 2 or ntb < 1 or nf < 1:
        return None
    tt = min(ntb, 128 // dsz)
    while True:
        shift = 4 if ssz >= 8 else 5
        while (2 << shift) * tt <= THREADS:
            shift += 1
        tc, stride = 1 << shift, tt | 1
        img = tc * stride
        slot, psb = nf * img * dsz, img * 8
        nslot = (LDS_BYTES - psb) // slot if psb < LDS_BYTES else 0
        if nslot >= 2:
            kw = min(nslot - 1, nlev - 1)
            return dict(tc_shift=shift, tt=tt, kw=kw, stride=stride, ppl=-(-tc * tt // THREADS), nct=-(-ncol // tc),
                        ntt=-(-ntb // tt), nwin=-(-(nlev - 1) // kw), lds=psb + (kw + 1) * slot)
        if tt == 1:
            return None
        tt = (tt + 1) // 2


def tile_cases():
    rows = list(itertools.product((1, 15, 1153, 3458), (2, 3, 26, 72, 128), (1, 37), (1, 3, 15, 16, 17, 30, 33, 92),
                                  (1, 4, 6, 8), ((8, 8), (8, 4), (4, 4))))
    rows = [(ncol, nlev, ntb, nf, d, s) for ncol, nlev, _, ntb, nf, (d, s) in rows]
    rows += [(777602, 72, 30, 4, 8, 8), (777602, 72, 30, 4, 4, 4), (48602, 72, 92, 4, 8, 8), (1 << 34, 2, 1, 1, 4, 4),
             (100, 72, 16, 40, 8, 8), (100, 72, 16, 400, 8, 4), (100, 1, 16, 4, 8, 8), (100, 5, 0, 4, 8, 8)]
    return sorted(set(rows))


@pytest.fixture(scope="module")
def library_tiles(tmp_path_factory):
    """The library's ingest_tile, compiled into tests/host/ingest_tile_main.cpp with AddressSanitizer + UBSan and run
    directly on every case."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")
    d = tmp_path_factory.mktemp("ingest_tile")
    exe = str(d / "ingest_tile_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "host", "ingest_tile_main.cpp"), "-o", exe], check=True)
    cases = tile_cases()
    path = str(d / "cases.txt")
    with open(path, "w") as fh:
        for c in cases:
            fh.write(" ".join(str(int(x)) for x in c) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return cases, out


def test_tile_mirror_equals_the_library(library_tiles):
    cases, out = library_tiles
    refused = 0
    for c, o in zip(cases, out):
        m = ingest_tile(*c)
        if m is None:
            assert o[0] == 0, c
            refused += 1
            continue
        names = ("tc_shift", "tt", "kw", "stride", "ppl", "nct", "ntt", "nwin", "lds")
        assert o[0] == 1 and dict(zip(names, o[1:])) == m, (c, o, m)
    assert refused == 4                                            # nlev = 1, ntb = 0; 40 and 400 fields: no two slots fit


def test_tile_invariants():
    """LDS within the budget; the tile has a pair for every lane slot and a lane slot for every pair; rows of at least
    128 bytes on the read side; every (column, level bracket, time) is covered exactly once; consecutive level
    windows share exactly one level, which stays in the ring (kw + 1 slots, level k in slot k mod (kw + 1))."""
    seen_kw, seen_ppl = set(), set()
    for c in tile_cases():
        m = ingest_tile(*c)
        if m is None:
            continue
        ncol, nlev, ntb, nf, dsz, ssz = c
        tc, tt, kw = 1 << m["tc_shift"], m["tt"], m["kw"]
        assert m["lds"] <= LDS_BYTES and m["lds"] == tc * m["stride"] * (8 + (kw + 1) * nf * dsz)
        assert m["stride"] % 2 == 1 and tt <= m["stride"] <= tt + 1
        assert tc * ssz >= 128 and 16 <= tc <= 256
        assert 1 <= tt <= min(ntb, 128 // dsz)
        assert (m["ppl"] - 1) * THREADS < tc * tt <= m["ppl"] * THREADS and m["ppl"] <= 32
        assert tc * tt >= THREADS // 2 or tc == 256                # short windows take more columns
        # columns and times: tiles cover 0 .. ncol and 0 .. ntb once
        assert (m["nct"] - 1) * tc < ncol <= m["nct"] * tc and (m["ntt"] - 1) * tt < ntb <= m["ntt"] * tt
        # level windows: brackets (k - 1, k), k = 1 .. nlev - 1, each in exactly one window; seams every kw levels
        assert 1 <= kw <= nlev - 1
        count = np.zeros(nlev, dtype=int)
        staged = np.zeros(nlev, dtype=int)
        for w in range(m["nwin"]):
            k0, k1 = w * kw, min(w * kw + kw, nlev - 1)
            assert k1 > k0
            count[k0 + 1:k1 + 1] += 1
            staged[(k0 if w == 0 else k0 + 1):k1 + 1] += 1         # level k0 of a later window is in the ring already
            slots = [(k % (kw + 1)) for k in range(k0, k1 + 1)]
            assert len(set(slots)) == len(slots)                   # the window's levels sit in different slots
        assert np.all(count[1:] == 1) and count[0] == 0
        assert np.all(staged == 1)                                 # every level is read from HBM once: no overlap re-read
        seen_kw.add(min(kw, 3))
        seen_ppl.add(m["ppl"])
    assert seen_kw == {1, 2, 3} and seen_ppl == {1, 2, 3, 4}


# ---- front end: refusals before any device -----------------------------------------------------------------------------
def _tiny(nt=2, nlev=8, ncol=5):
    hyam, hybm = hybrid_levels(nlev)
    f = np.zeros((nt, nlev, ncol))
    lat = np.linspace(-80, 80, ncol)
    ps = np.full((nt, ncol), 1e5)
    return f, lat, ps, dict(plev=[500.0], hyam=hyam, hybm=hybm)


def test_from_model_levels_refuses_other_orders_and_shapes_before_a_device():
    from pytemdiags_amd import LabeledArray, TEMDiagnostics
    f, lat, ps, kw = _tiny()
    fm = TEMDiagnostics.from_model_levels
    for dims in (("time", "ncol", "lev"), ("lev", "time", "ncol"), ("ncol", "time", "lev"), ("lev", "ncol", "time"),
                 ("time", "lev"), ("time", "lev", "col"), ("time", "ncol", "ncol")):
        with pytest.raises(ValueError, match=r"\(ncol, vert, time\).*\(time, vert, ncol\)"):
            fm(f, f, f, f, lat, ps=ps, dims=dims, **kw)
    lab = LabeledArray(f, ("time", "ncol", "lev"), {}, name="U")
    with pytest.raises(ValueError, match=r"\(ncol, vert, time\).*\(time, vert, ncol\)"):
        fm(lab, lab, lab, lab, lat, ps=ps, **kw)
    # ps of the wrong shape for the order
    with pytest.raises(ValueError, match=r"ps has shape \(5, 2\), expected \(2, 5\)"):
        fm(f, f, f, f, lat, ps=np.ascontiguousarray(ps.T), dims=TM, **kw)
    with pytest.raises(ValueError, match="p_model has shape"):
        fm(f, f, f, f, lat, p_model=np.zeros((5, 8, 2)), dims=TM, plev=[500.0])
    # time-major input is taken as it lies: no view that would need a copy
    g = np.zeros((5, 8, 2)).transpose(2, 1, 0)
    assert g.shape == f.shape and not g.flags.c_contiguous
    with pytest.raises(ValueError, match="not C-contiguous"):
        fm(f, g, f, f, lat, ps=ps, dims=TM, **kw)
    with pytest.raises(ValueError, match="not C-contiguous"):
        fm(f, f, f, f, lat, ps=np.full((5, 2), 1e5).T, dims=TM, **kw)
    # mixed kinds, mixed orders, shapes, dtypes
    with pytest.raises(ValueError, match="same kind"):
        fm(LabeledArray(f, TM, {}, name="U"), f, f, f, lat, ps=ps, dims=TM, **kw)
    with pytest.raises(ValueError, match="same order"):
        fm(LabeledArray(f, TM, {}), LabeledArray(np.zeros((5, 8, 2)), ("ncol", "lev", "time"), {}),
           LabeledArray(f, TM, {}), LabeledArray(f, TM, {}), lat, ps=ps, **kw)
    with pytest.raises(ValueError, match="field 1 has shape"):
        fm(f, np.zeros((2, 8, 6)), f, f, lat, ps=ps, dims=TM, **kw)
    with pytest.raises(ValueError, match="float64 or float32"):
        fm(f, f.astype(np.int32), f, f, lat, ps=ps, dims=TM, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        fm(f, f, f, f, lat, dims=TM, **kw)
    with pytest.raises(ValueError, match="hyam / hybm have"):
        fm(f, f, f, f, lat, ps=ps, dims=TM, plev=[500.0], hyam=kw["hyam"][:5], hybm=kw["hybm"][:5])
    with pytest.raises(ValueError, match="not strictly increasing"):
        fm(f, f, f, f, lat, ps=ps, dims=TM, plev=[500.0], hyam=kw["hyam"][::-1], hybm=kw["hybm"][::-1])
    with pytest.raises(ValueError, match="method"):
        fm(f, f, f, f, lat, ps=ps, dims=TM, interp="cubic", **kw)
    with pytest.raises(ValueError, match="time_block"):
        fm(f, f, f, f, lat, ps=ps, dims=TM, time_block=0, **kw)
    with pytest.raises(NotImplementedError, match="tracers"):
        fm(f, f, f, f, lat, ps=ps, dims=TM, q=f, missing="mask", **kw)
    with pytest.raises(ValueError, match="missing"):
        fm(f, f, f, f, lat, ps=ps, dims=TM, missing="bogus", **kw)


def test_finite_range_reads_a_host_record_block_wise(tmp_path):
    from pytemdiags_amd.vertical import finite_range
    rng = np.random.default_rng(0)
    ps = rng.uniform(5e4, 1.05e5, (37, 11)).astype(np.float32)
    ps[3, 4] = np.nan
    ps[30, 1] = np.inf
    fin = ps[np.isfinite(ps)]
    assert finite_range(ps, rows=5) == (float(fin.min()), float(fin.max())) == finite_range(ps)
    m = np.memmap(str(tmp_path / "ps.bin"), dtype=np.float32, mode="w+", shape=ps.shape)
    m[:] = ps
    assert finite_range(m, rows=4) == finite_range(ps)
    import torch
    assert finite_range(torch.as_tensor(ps), rows=7) == finite_range(ps)
    assert finite_range(np.full((3, 2), np.nan)) is None


def test_host_blocks_keeps_its_defaults():
    """The re-layout source of a blocked run is the class it was: same constructor call, same timing keys."""
    import inspect
    from pytemdiags_amd import layout, vertical
    p = inspect.signature(layout.HostBlocks.__init__).parameters
    assert list(p)[:5] == ["self", "arrays", "device", "flip_lev", "work"]
    assert p["step"].default is None and p["step_name"].default == "relayout_ms"
    for cls in (layout.HostBlocks, layout.DeviceBlocks, vertical.HostRecordBlocks, vertical.DeviceRecordBlocks):
        for name in ("start", "get", "after_launch", "done", "close"):
            assert callable(getattr(cls, name)), (cls, name)


# ---- the gate --------------------------------------------------------------------------------------------------------
def test_fused_gate_is_backed_by_a_committed_measurement():
    """``vertical.FUSED_RECORDS`` may switch the fused call on for a dtype only if profiles/ingest_bench_mi355x.json
    exists and shows it no slower than the chain, with equal bits, in every leg of that dtype."""
    from pytemdiags_amd import vertical
    assert set(vertical.FUSED_RECORDS) == {"float64", "float32"}
    assert all(isinstance(v, bool) for v in vertical.FUSED_RECORDS.values())
    path = os.path.join(ROOT, "profiles", "ingest_bench_mi355x.json")
    for name, on in vertical.FUSED_RECORDS.items():
        if not on:
            continue
        assert os.path.exists(path), "FUSED_RECORDS[%r] is on without a measurement" % name
        legs = [r for r in json.load(open(path))["legs"] if r.get("dtype") == name]
        shapes = {(r["ncol"], r["nlev"], r["nplev"], r["nt"]) for r in legs}
        assert (777602, 72, 37, 30) in shapes
        assert name == "float32" or {(777602, 72, 72, 16), (48602, 72, 37, 92)} <= shapes
        assert all(r["equal_to_chain"] is True and r["chain_over_fused_time"] >= 1.0 for r in legs), name
