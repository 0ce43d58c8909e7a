"""temxv_interp where the first tests of it did not go: every regime of the slab geometry, exact ties at segment seams
and at the column edges, pointers that are only element aligned (with guard zones round every output), field counts
1..13, the table cache past its 16 sets, the map selection errors, and non-positive pressures in log mode.

The reference everywhere is test_vertical_host.interp_ref; the comparison is test_gpu_vertical.check, with nothing
excluded from the NaN pattern.  The fixtures (rough columns, tie columns, the mirror of vert_slab_shape) live in
test_vertical_host.py, which also asserts on the CPU what each of them is meant to contain."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_vertical import check
from test_vertical_host import (SWEEP, TIE_CASES, amplification, hybrid_pressure, interp_ref, rough_case, rough_targets,
                                slab_shape, sweep_id, sweep_ncol, tie_case, tie_ncol)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MAPS = ("time", "slab")


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_scaled(out, ref, dtype, what, a):
    """check(), with the fp64 bound scaled by A / 300 for the two 1000-level cases (A from the fixture)."""
    if a < 300 or dtype != np.float64:
        return check(out, ref, dtype, what)
    assert np.array_equal(np.isnan(out), np.isnan(ref)), what
    fin = np.isfinite(ref)
    assert out.dtype == dtype and fin.any()
    d = float(np.max(np.abs(out[fin] - ref[fin])))
    bound = 1e-12 * a / 300.0 * float(np.max(np.abs(ref[fin])))
    print("%s: max|d| = %.3e, bound %.3e (A = %.0f)" % (what, d, bound, a))
    assert d <= bound, (what, d, bound)


def run_maps(monkeypatch, maps, fields, plev_hpa, **kw):
    from pytemdiags_amd import interp_to_pressure
    got = {}
    try:
        for m in maps:
            if m is None:
                monkeypatch.delenv("TEMXV_MAP", raising=False)
            else:
                monkeypatch.setenv("TEMXV_MAP", m)
            got[m] = interp_to_pressure(fields, plev_hpa, **kw)
    finally:
        monkeypatch.delenv("TEMXV_MAP", raising=False)
    return got


def pressure_kw(c, **more):
    if c["P"] is not None:
        return dict(p=c["P"], **more)
    return dict(ps=c["ps"], hyam=c["hyam"], hybm=c["hybm"], **more)


# ---- a. slab geometry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SWEEP, ids=sweep_id)
def test_slab_geometry_sweep(case, monkeypatch):
    """Every regime of vert_slab_shape (test_vertical_host.test_sweep_shapes_hit_the_regimes_they_name asserts which),
    in both maps where the slab map applies, both edge policies, and both methods except on the three largest shapes."""
    nf, nlev, nt, nplev, dtype, pmode, pdt, res, claim = case
    ncol = sweep_ncol(case)
    c = rough_case(ncol, nlev, nt, nf, pmode, dtype, pdt)
    plev = rough_targets(nplev)
    maps = MAPS if claim is not None else ("time", None)     # no slab: the default must fall back to the time map
    if claim == {}:
        maps = MAPS + (None,)                                # the switch points: the default map as well
    for method in ("log", "linear") if nlev < 128 else ("log",):
        a = amplification(c["p"], method)
        for edge in ("nan", "hold"):
            got = run_maps(monkeypatch, maps, c["f"], plev, method=method, edge=edge, **pressure_kw(c))
            for i in range(nf):
                ref = interp_ref(c["f"][i], c["p"], plev * 100.0, method, edge, psurf=c["psurf"])
                check_scaled(got[maps[0]][i], ref, dtype, "%s %s %s f%d" % (sweep_id(case), method, edge, i), a)
                for m in maps[1:]:
                    assert same(got[maps[0]][i], got[m][i]), (sweep_id(case), method, edge, i, m)


# ---- b. exact ties ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev,nt,pmode,nf,ps_dtype", TIE_CASES,
                         ids=["%s-nlev%d-nt%d-ps_%s" % (c[2], c[0], c[1], np.dtype(c[4]).name) for c in TIE_CASES])
def test_exact_ties_at_seams_levels_and_surface(nlev, nt, pmode, nf, ps_dtype, monkeypatch):
    """Targets that are the same fp64 number as a level: level 0, every segment seam of the slab map, two other
    levels, the bottom level and (hybrid) the surface in a third of the columns.  p_{k-1} < pt <= p_k decides both
    the bracket and the lane that owns the target; pt <= psurf decides what is held."""
    c, intended = tie_case(nlev, nt, tie_ncol(nlev, nt, pmode, nf), nf, ps_dtype)
    assert intended >= 100
    sh = slab_shape(nf, nlev, nt, c["pt"].size, 8, 0 if pmode == "hybrid" else 8)
    assert tuple(range(sh["seg"], nlev - 1, sh["seg"])) == c["seams"]
    if pmode == "hybrid":
        kw = dict(ps=c["ps"], hyam=c["hyam"], hybm=c["hybm"], p0=c["p0"])
        psurf = c["psurf"]
    else:
        kw = dict(p=c["p"])
        psurf = None
    pt = c["pt"]
    j_of = {k: int(np.flatnonzero(pt == c["H"][k] * 100.0 / 64.0)[0]) for k in c["tied_levels"]}
    for method in ("log", "linear"):
        for edge in ("nan", "hold"):
            got = run_maps(monkeypatch, MAPS, c["f"], c["plev_hpa"], method=method, edge=edge, **kw)
            for i in range(nf):
                what = "ties %s nlev=%d %s %s f%d" % (pmode, nlev, method, edge, i)
                ref = interp_ref(c["f"][i], c["p"], pt, method, edge, psurf=psurf)
                out = got["time"][i]
                check(out, ref, np.float64, what)
                assert same(out, got["slab"][i]), what
                scale = float(np.max(np.abs(c["f"][i])))
                for k, j in j_of.items():             # a tie on level k returns level k's value
                    cols = slice(None) if k < {26: 16, 13: 9}[nlev] else c["star"]
                    assert np.max(np.abs(out[cols, j, :] - c["f"][i][cols, k, :])) <= 1e-12 * scale, (what, k)
                assert np.all(np.isfinite(out[:, j_of[0], :])) and np.all(np.isfinite(out[c["star"], j_of[nlev - 1], :]))
                if pmode == "hybrid":                 # pt == ps: held under "hold", outside the column under "nan"
                    js = int(np.flatnonzero(pt == 99500.0)[0])
                    if edge == "hold":
                        assert np.array_equal(out[c["star"], js, :], c["f"][i][c["star"], -1, :])
                    else:
                        assert np.all(np.isnan(out[c["star"], js, :]))


# ---- c. element-aligned pointers and guard zones, through the C ABI -----------------------------------------------
GUARD = 64


def place(arena_dtype, sizes, offsets, sentinel):
    """One arena holding len(sizes) arrays, each starting `offsets[i]` elements past a 16-byte boundary with at least
    GUARD sentinel elements on both sides.  Returns (arena tensor, element offsets)."""
    per16 = 16 // np.dtype(arena_dtype).itemsize
    at, cur = [], GUARD
    for n, off in zip(sizes, offsets):
        start = -(-cur // per16) * per16 + off
        at.append(start)
        cur = start + n + GUARD
    tdt = torch.float64 if arena_dtype == np.float64 else torch.float32
    arena = torch.full((cur + per16,), sentinel, dtype=tdt, device="cuda:0")
    assert arena.data_ptr() % 16 == 0
    return arena, at


@pytest.mark.parametrize("pmode", ["hybrid", "field"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("nf,nlev,nt,nplev", [(4, 6, 3, 5), (3, 5, 1, 3)])
def test_c_abi_element_aligned_pointers_and_nothing_written_outside_dst(nf, nlev, nt, nplev, dtype, pmode, monkeypatch):
    from pytemdiags_amd import _vert
    lib = _vert.load()
    size = np.dtype(dtype).itemsize
    sh = slab_shape(nf, nlev, nt, nplev, size, 0 if pmode == "hybrid" else size)
    ncol = 3 * sh["cw"] + 5
    c = rough_case(ncol, nlev, nt, nf, pmode, dtype, dtype, seed=3)
    plev = rough_targets(nplev)
    pt = np.ascontiguousarray(plev * 100.0)
    big = 1e300 if dtype == np.float64 else 1e30
    dst_fill = -3e200 if dtype == np.float64 else -3e20
    nin, nout = ncol * nlev * nt, ncol * nplev * nt
    src_arena, src_at = place(dtype, [nin] * nf, [(f % 3) + 1 for f in range(nf)], big)
    dst_arena, dst_at = place(dtype, [nout] * nf, [((f + 1) % 3) + 1 for f in range(nf)], dst_fill)
    pin = c["ps"] if pmode == "hybrid" else c["P"]
    p_arena, p_at = place(dtype, [pin.size], [3], big)
    for f in range(nf):
        src_arena[src_at[f]:src_at[f] + nin] = torch.as_tensor(c["f"][f].ravel(), device="cuda:0")
    p_arena[p_at[0]:p_at[0] + pin.size] = torch.as_tensor(pin.ravel(), device="cuda:0")
    for arena, ats, offs in ((src_arena, src_at, [(f % 3) + 1 for f in range(nf)]),
                             (dst_arena, dst_at, [((f + 1) % 3) + 1 for f in range(nf)]), (p_arena, p_at, [3])):
        for a, off in zip(ats, offs):                # off elements past a 16-byte boundary, guards on both sides
            assert (arena.data_ptr() + a * size) % 16 == (off * size) % 16 and a >= GUARD
    before = dst_arena.clone()
    outside = torch.ones(dst_arena.numel(), dtype=torch.bool, device="cuda:0")
    for a in dst_at:
        outside[a:a + nout] = False
    idt = torch.int64 if dtype == np.float64 else torch.int32
    dp = C.POINTER(C.c_double)
    src = (C.c_void_p * nf)(*[src_arena.data_ptr() + a * size for a in src_at])
    dst = (C.c_void_p * nf)(*[dst_arena.data_ptr() + a * size for a in dst_at])
    hy = (c["hyam"].ctypes.data_as(dp), c["hybm"].ctypes.data_as(dp)) if pmode == "hybrid" else (None, None)
    code = 0 if dtype == np.float64 else 1
    for method, edge in (("log", "hold"), ("linear", "nan")):
        got = {}
        for m in MAPS:
            dst_arena.copy_(before)
            monkeypatch.setenv("TEMXV_MAP", m)
            rc = lib.temxv_interp(0, nf, src, dst, code, ncol, nlev, nt, nplev, pt.ctypes.data_as(dp),
                                  0 if pmode == "hybrid" else 1, hy[0], hy[1], 1e5,
                                  C.c_void_p(p_arena.data_ptr() + p_at[0] * size), code,
                                  _vert.METHODS[method], _vert.EDGES[edge], None)
            monkeypatch.delenv("TEMXV_MAP")
            assert rc == 0, lib.temx_last_error()
            torch.cuda.synchronize()
            # every guard element of the destination arena keeps its bits
            assert torch.equal(dst_arena.view(idt)[outside], before.view(idt)[outside]), (m, method, edge)
            got[m] = [dst_arena[a:a + nout].cpu().numpy().reshape(ncol, nplev, nt) for a in dst_at]
        for f in range(nf):
            what = "unaligned %s %s nf%d nlev%d %s %s f%d" % (pmode, np.dtype(dtype).name, nf, nlev, method, edge, f)
            ref = interp_ref(c["f"][f], c["p"], pt, method, edge, psurf=c["psurf"])
            check(got["time"][f], ref, dtype, what)
            assert same(got["time"][f], got["slab"][f]), what
            fin = np.isfinite(got["slab"][f])
            assert np.all(np.abs(got["slab"][f][fin]) < 1e3), what      # neither sentinel, nor anything computed from one


# ---- d. field counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [3, 20])
def test_every_field_count_equals_the_field_alone(nt, monkeypatch):
    """nf = 1..8 in one launch (both kernel templates, nf below the template's count), 9 and 13 fields split over two
    launches: each output is the bits of that field interpolated alone.  nt = 3 takes the slab map, nt = 20 lanes along
    time."""
    from pytemdiags_amd import interp_to_pressure
    nlev, nplev = 9, 6
    sh = slab_shape(8, nlev, nt, nplev, 8, 0)
    ncol = max(3 * sh["cw"] + 2, 600 // nt)           # three workgroups in either map
    c = rough_case(ncol, nlev, nt, 13, "hybrid", seed=4)
    plev = rough_targets(nplev)
    kw = pressure_kw(c, edge="hold")
    alone = [interp_to_pressure(x, plev, **kw) for x in c["f"]]
    for i in range(13):
        check(alone[i], interp_ref(c["f"][i], c["p"], plev * 100.0, "log", "hold", psurf=c["psurf"]), np.float64,
              "alone nt=%d f%d" % (nt, i))
    for nf in list(range(1, 9)) + [9, 13]:
        out = interp_to_pressure(c["f"][:nf], plev, **kw)
        assert len(out) == nf
        for i in range(nf):
            assert same(out[i], alone[i]), (nt, nf, i)
    # the last field of a launch sits in the last used slot of the template: pick it from the other end too
    out = interp_to_pressure(c["f"][12:4:-1], plev, **kw)
    for o, i in zip(out, range(12, 4, -1)):
        assert same(o, alone[i]), (nt, i)


def test_mixed_precision_field_list_promotes_to_fp64():
    from pytemdiags_amd import interp_to_pressure
    c = rough_case(150, 9, 3, 5, "field", seed=5)
    plev = rough_targets(6)
    mixed = [x.astype(np.float32) if i % 2 else x for i, x in enumerate(c["f"])]
    up = [x.astype(np.float64) for x in mixed]
    out = interp_to_pressure(mixed, plev, p=c["P"], edge="hold")
    ref = interp_to_pressure(up, plev, p=c["P"], edge="hold")
    for i in range(5):
        assert out[i].dtype == np.float64 and same(out[i], ref[i]), i
        check(out[i], interp_ref(up[i], c["p"], plev * 100.0, "log", "hold"), np.float64, "mixed f%d" % i)
    all32 = interp_to_pressure([x.astype(np.float32) for x in c["f"]], plev, p=c["P"], edge="hold")
    assert all(x.dtype == np.float32 for x in all32)


# ---- e. table cache -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side_stream", [False, True], ids=["current_stream", "side_stream"])
def test_table_cache_past_sixteen_sets_and_back(side_stream):
    """vert_tables keeps 16 uploaded sets: twenty distinct sets evict the first four, and a call that returns to an
    evicted set has to upload it again.  The sets differ by the target values or by the method alone."""
    from pytemdiags_amd import interp_to_pressure
    c = rough_case(40, 5, 2, 2, "hybrid", seed=6 + side_stream)
    dev = [torch.as_tensor(x, device="cuda:0") for x in c["f"]]
    psd = torch.as_tensor(c["ps"], device="cuda:0")
    base = rough_targets(4)
    sets = []
    for n in range(10):
        plev = base * (1.0 + 0.003 * (n + 10 * side_stream))           # same sizes, different values
        sets += [(plev, "log"), (plev, "linear")]                       # ... and the same values, another method
    stream = torch.cuda.Stream(device="cuda:0") if side_stream else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    first = []
    with torch.cuda.stream(stream):
        for plev, method in sets + sets[:3]:
            out = interp_to_pressure(dev, plev, ps=psd, hyam=c["hyam"], hybm=c["hybm"], method=method, edge="hold")
            first.append([o.cpu().numpy() for o in out])
    stream.synchronize()
    for n, (plev, method) in enumerate(sets + sets[:3]):
        for i in range(2):
            ref = interp_ref(c["f"][i], c["p"], plev * 100.0, method, "hold", psurf=c["psurf"])
            check(first[n][i], ref, np.float64, "table set %d %s f%d" % (n, method, i))
    for n in range(3):
        for i in range(2):
            assert same(first[20 + n][i], first[n][i]), n


# ---- f. map selection ---------------------------------------------------------------------------------------------
def test_forced_slab_map_that_cannot_apply_is_refused(monkeypatch):
    from pytemdiags_amd import _vert, interp_to_pressure
    lib = _vert.load()
    ncol, nlev, nt, nplev = 7, 5, 65, 3
    assert slab_shape(1, nlev, nt, nplev, 8, 0) is None and slab_shape(1, nlev, 64, nplev, 8, 0) is not None
    c = rough_case(ncol, nlev, nt, 1, "hybrid", seed=8)
    plev = rough_targets(nplev)
    ref = interp_ref(c["f"][0], c["p"], plev * 100.0, psurf=c["psurf"])
    monkeypatch.setenv("TEMXV_MAP", "slab")
    with pytest.raises(_vert.TemxError, match="does not fit") as err:
        interp_to_pressure(c["f"][0], plev, **pressure_kw(c))
    assert err.value.code == -6
    # the C ABI: TEMX_EUNSUPPORTED, and nothing was launched
    x = torch.as_tensor(c["f"][0], device="cuda:0")
    ps = torch.as_tensor(c["ps"], device="cuda:0")
    y = torch.full((ncol, nplev, nt), 123.0, dtype=torch.float64, device="cuda:0")
    dp = C.POINTER(C.c_double)
    pt = np.ascontiguousarray(plev * 100.0)
    args = (0, 1, (C.c_void_p * 1)(x.data_ptr()), (C.c_void_p * 1)(y.data_ptr()), 0, ncol, nlev, nt, nplev,
            pt.ctypes.data_as(dp), 0, c["hyam"].ctypes.data_as(dp), c["hybm"].ctypes.data_as(dp), 1e5,
            C.c_void_p(ps.data_ptr()), 0, 0, 0, None)
    assert lib.temxv_interp(*args) == -6 and b"does not fit" in lib.temx_last_error()
    torch.cuda.synchronize()
    assert bool((y == 123.0).all())
    # an unknown value behaves as unset: the call goes through (on the time map, the only one for 65 times)
    monkeypatch.setenv("TEMXV_MAP", "bogus")
    bogus = interp_to_pressure(c["f"][0], plev, **pressure_kw(c))
    assert lib.temxv_interp(*args) == 0
    torch.cuda.synchronize()
    monkeypatch.delenv("TEMXV_MAP")
    unset = interp_to_pressure(c["f"][0], plev, **pressure_kw(c))
    check(unset, ref, np.float64, "TEMXV_MAP unset nt=65")
    assert same(bogus, unset) and same(y.cpu().numpy(), unset)
    # ... and at a short row, where unset means the slab map
    s = rough_case(300, 9, 3, 2, "field", seed=9)
    got = run_maps(monkeypatch, ("bogus", None, "slab"), s["f"], plev, p=s["P"])
    for i in range(2):
        check(got["bogus"][i], interp_ref(s["f"][i], s["p"], plev * 100.0), np.float64, "TEMXV_MAP=bogus f%d" % i)
        assert same(got["bogus"][i], got[None][i]) and same(got["bogus"][i], got["slab"][i])


def test_a_refused_device_leaves_no_error_behind_for_the_caller():
    """temxv_interp on a device that does not exist returns TEMX_EHIP.  HIP keeps a failed call as the thread's last
    error until it is read; the library reads it, so the caller's next launch (torch checks after its own) is clean.
    Found by running test_vertical_host.py, which makes such a call, in one process with the GPU tests."""
    from pytemdiags_amd import _vert, interp_to_pressure
    lib = _vert.load()
    torch.cuda.synchronize()
    x = torch.zeros(4 * 3 * 2, dtype=torch.float64, device="cuda:0")
    y = torch.zeros(4 * 2 * 2, dtype=torch.float64, device="cuda:0")
    ps = torch.full((4, 2), 1e5, dtype=torch.float64, device="cuda:0")
    dp = C.POINTER(C.c_double)
    plev = (C.c_double * 2)(5e4, 7e4)
    hy = (C.c_double * 3)(0.1, 0.2, 0.3)
    rc = lib.temxv_interp(99, 1, (C.c_void_p * 1)(x.data_ptr()), (C.c_void_p * 1)(y.data_ptr()), 0, 4, 3, 2, 2, plev,
                          0, hy, hy, 1e5, C.c_void_p(ps.data_ptr()), 0, 0, 0, None)
    assert rc == -2 and b"hipSetDevice" in lib.temx_last_error()
    z = torch.arange(6, device="cuda:0", dtype=torch.float64).reshape(2, 3).to(torch.float32).contiguous() + 1.0
    torch.cuda.synchronize()
    assert float(z.sum()) == 21.0
    c = rough_case(20, 5, 2, 1, "hybrid", seed=12)
    plev_hpa = rough_targets(4)
    out = interp_to_pressure(c["f"][0], plev_hpa, **pressure_kw(c))
    check(out, interp_ref(c["f"][0], c["p"], plev_hpa * 100.0, psurf=c["psurf"]), np.float64, "after a refused device")


# ---- non-positive pressure ----------------------------------------------------------------------------------------
def test_non_positive_pressure_is_a_bad_column_in_log_mode_only(monkeypatch):
    """Interface levels start at p_0 = 0.  method="log": the (column, time) is NaN throughout, its neighbours are
    untouched; method="linear" interpolates it like any finite increasing column."""
    nlev, nt, nplev, nf = 9, 3, 6, 2
    ncol = 3 * slab_shape(nf, nlev, nt, nplev, 8, 8)["cw"] + 4
    c = rough_case(ncol, nlev, nt, nf, "field", seed=10)
    plev = rough_targets(nplev)
    p = c["p"].copy()
    zero = [(0, 0), (5, 1), (ncol // 2, 2), (ncol - 1, 0)]
    for i, t in zero:
        p[i, 0, t] = 0.0
    p[9, 0, :] = -2.0
    for method in ("log", "linear"):
        for edge in ("nan", "hold"):
            got = run_maps(monkeypatch, MAPS, c["f"], plev, p=p, method=method, edge=edge)
            clean = run_maps(monkeypatch, ("slab",), c["f"], plev, p=c["p"], method=method, edge=edge)["slab"]
            for f in range(nf):
                what = "p0 = 0 %s %s f%d" % (method, edge, f)
                check(got["time"][f], interp_ref(c["f"][f], p, plev * 100.0, method, edge), np.float64, what)
                assert same(got["time"][f], got["slab"][f]), what
                hit = np.zeros(got["slab"][f].shape, bool)
                for i, t in zero:
                    hit[i, :, t] = True
                hit[9] = True
                if method == "log":
                    assert np.all(np.isnan(got["slab"][f][hit])), what
                    assert same(got["slab"][f][~hit], clean[f][~hit]), what      # neighbours untouched
                else:
                    assert np.isfinite(got["slab"][f][hit]).any(), what
    # hybrid: hyam[0] = hybm[0] = 0 puts p_0 = 0 into every column
    h = rough_case(ncol, nlev, nt, nf, "hybrid", seed=11)
    h["hyam"][0] = h["hybm"][0] = 0.0
    ph = hybrid_pressure(h["hyam"], h["hybm"], h["psurf"])
    for method in ("log", "linear"):
        got = run_maps(monkeypatch, MAPS, h["f"], plev, method=method, edge="hold", **pressure_kw(h))
        for f in range(nf):
            ref = interp_ref(h["f"][f], ph, plev * 100.0, method, "hold", psurf=h["psurf"])
            assert same(got["time"][f], got["slab"][f])
            if method == "log":
                assert np.all(np.isnan(ref)) and np.all(np.isnan(got["slab"][f]))
            else:
                check(got["slab"][f], ref, np.float64, "hybrid p0 = 0 linear f%d" % f)
