"""Time-mean TEM on the MI355X: the time sum (temxc_time_sum), the epilogue on supplied zonal means
(temxc_tem_from_zonal_means) and ``TEMDiagnostics(..., climatology=True)``.

Bounds.
  * time sum against ``np.sum(x.astype(float64), -1)``, per row: |delta| <= 2 nt 2^-53 sum_t |x_t| -- any order of
    fp64 additions is within (nt - 1) 2^-53 sum|x| of the exact sum, so two orders are within twice that; bitwise at
    nt = 1.  Blocks accumulated against the whole: the same bound.
  * front end against the numpy oracle: 1e-10 field-normalised for fp64 (the project's oracle bound), 2e-5 for fp32
    fields; transient quantities and the four flux-linear results of every set are normalised by the TOTAL's maximum,
    because they are differences.  Stationary + transient = total for the four linear results: 1e-12.  A blocked run
    against the whole run: 1e-11 (the project's bound between blocks and the whole); one block: bit for bit.  The two
    time-sum paths against each other: 1e-12 (the time-sum bound carried to the results).
References: stationary set ``TEMOracle(time-mean fields)``; total set ``TEMOracle.from_zonal_means`` of the time mean of
the oracle's per-snapshot zonal means; transient set the same with the difference of the fluxes
(tests/test_clim_host.py, clim_reference)."""
import ctypes as C

import numpy as np
import pytest

from oracle import tem_oracle as orc
from test_clim_host import FLUXES, LINEAR, ZM7, clim_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
SETS = ("total", "stationary", "transient")
CANARY = -7.25e300
NCOLS, NLEVS = (1, 37, 866), (1, 3, 6)
_cache = {}


def _names():
    from pytemdiags_amd import _lib
    return _lib.RESULT_NAMES, _lib.ZONAL_NAMES


def switch(dtype):
    from pytemdiags_amd import _clim
    return _clim.switch_nt(np.dtype(dtype).itemsize)


def nts_of(dtype):
    s = switch(dtype)
    return sorted({1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 129, s - 1, s, s + 1, 1000})


def small_plan():
    """A plan to call the methods on: the time sum needs none of its tables."""
    if "plan" not in _cache:
        from pytemdiags_amd import engine, synth
        lat, _ = synth.cubed_sphere_gll(4)
        _cache["plan"] = engine.Plan(lat, orc.zm_latitudes(1), 10, device=0)
    return _cache["plan"]


def bound(x):
    """2 nt 2^-53 sum_t |x_t| per row, and the reference."""
    x64 = np.asarray(x, dtype=np.float64)
    return np.sum(x64, -1), 2.0 * x.shape[-1] * 2.0 ** -53 * np.sum(np.abs(x64), -1)


def off_by_one(x):
    """A device copy of ``x`` that starts one element into a larger buffer: nothing is 16-byte aligned by design."""
    t = torch.as_tensor(np.ascontiguousarray(x))
    buf = torch.empty(t.numel() + 3, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + t.element_size()
    return v


class Guarded:
    """fp64 accumulators ``[ncol][nlev]``, each a view one element into a buffer of its own full of canaries."""

    def __init__(self, n, ncol, nlev):
        rows = ncol * nlev
        self.bufs = [torch.full((rows + 4,), CANARY, dtype=torch.float64, device=DEV) for _ in range(n)]
        self.acc = [b[1:1 + rows].view(ncol, nlev) for b in self.bufs]
        self.rows = rows

    def check(self):
        for b in self.bufs:
            edge = torch.cat([b[:1], b[1 + self.rows:]]).cpu().numpy()
            assert np.all(edge == CANARY), "a canary next to an accumulator was overwritten"

    def numpy(self):
        return [a.cpu().numpy().copy() for a in self.acc]


def time_sum(fields, accumulate_into=None):
    """-> (sums as numpy, the Guarded accumulators); sources and accumulators unaligned, canaries checked."""
    plan = small_plan()
    ncol, nlev, _ = fields[0].shape
    g = accumulate_into or Guarded(len(fields), ncol, nlev)
    out = plan.time_sum([off_by_one(x) for x in fields], acc=g.acc, accumulate=accumulate_into is not None)
    assert all(o is a for o, a in zip(out, g.acc))
    torch.cuda.synchronize()
    g.check()
    return g.numpy(), g


# ---- temxc_time_sum -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_time_sum_parity_every_shape_unaligned_with_canaries(dtype):
    rng = np.random.default_rng(11)
    worst = 0.0
    for nt in nts_of(dtype):
        big = (rng.standard_normal((NCOLS[-1] * NLEVS[-1], nt)) * 10.0 ** rng.integers(-3, 4, (NCOLS[-1] * NLEVS[-1], 1))).astype(dtype)
        for ncol in NCOLS:
            for nlev in NLEVS:
                x = big[:ncol * nlev].reshape(ncol, nlev, nt)
                (got,), _ = time_sum([x])
                ref, tol = bound(x)
                assert got.shape == (ncol, nlev) and got.dtype == np.float64
                assert np.all(np.abs(got - ref) <= tol), (nt, ncol, nlev, float(np.max(np.abs(got - ref) - tol)))
                worst = max(worst, float(np.max(np.abs(got - ref) / np.maximum(tol, 1e-300))))
                if nt == 1:
                    assert got.tobytes() == x[..., 0].astype(np.float64).tobytes()
                (again,), _ = time_sum([x])                              # repeated calls: identical bits
                assert again.tobytes() == got.tobytes()
                # equal rows give equal bits whatever ncol, nlev and the row's position: the rows of the largest case
                key = (np.dtype(dtype).name, nt)
                if (ncol, nlev) == (NCOLS[-1], NLEVS[-1]):
                    for (c, k), small in _cache.pop(key, {}).items():
                        assert small.tobytes() == got.reshape(-1)[:c * k].tobytes(), (nt, c, k)
                else:
                    _cache.setdefault(key, {})[(ncol, nlev)] = got.reshape(-1)
    print("%s: worst |delta| / bound %.3f over nt in %s" % (np.dtype(dtype).name, worst, nts_of(dtype)))


def test_time_sum_bitwise_at_nt_1_keeps_signed_zero_and_subnormals():
    x = np.array([[-0.0, 0.0, 5e-324, -1.5, np.float64(np.float32(1e-45))]]).reshape(1, 5, 1)
    (got,), _ = time_sum([x])
    assert got.tobytes() == x[..., 0].tobytes()
    x32 = np.array([-0.0, 1e-45, 3.25], dtype=np.float32).reshape(3, 1, 1)
    (got,), _ = time_sum([x32])
    assert got.tobytes() == x32[..., 0].astype(np.float64).tobytes()


@pytest.mark.parametrize("nt", [17, 300, 1000])
def test_time_sum_mixed_dtypes_eight_fields_one_call(nt):
    """nt = 300 lies between the two switch points: the fp64 fields take the long rows, the fp32 fields are staged."""
    assert switch(np.float64) <= 300 < switch(np.float32)
    rng = np.random.default_rng(nt)
    fields = [rng.standard_normal((37, 3, nt)).astype(np.float32 if f % 2 else np.float64) for f in range(8)]
    got, _ = time_sum(fields)
    for f, (x, g) in enumerate(zip(fields, got)):
        ref, tol = bound(x)
        assert np.all(np.abs(g - ref) <= tol), f
        (alone,), _ = time_sum([x])                  # the sum of a row does not depend on what else the call carries
        assert alone.tobytes() == g.tobytes(), f


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_time_sum_non_finite_values_poison_their_own_row_only(dtype):
    for nt in (17, switch(dtype) + 1):
        x = np.random.default_rng(5).standard_normal((37, 3, nt)).astype(dtype)
        (clean,), _ = time_sum([x])
        y = x.copy()
        y[5, 1, nt // 2] = np.nan
        y[20, 2, 0] = np.inf
        y[36, 2, nt - 1] = -np.inf
        (got,), _ = time_sum([y])
        assert np.isnan(got[5, 1]) and got[20, 2] == np.inf and got[36, 2] == -np.inf
        hit = np.zeros((37, 3), dtype=bool)
        hit[5, 1] = hit[20, 2] = hit[36, 2] = True
        assert np.all(np.isfinite(got[~hit])) and got[~hit].tobytes() == clean[~hit].tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_time_sum_permuting_rows_permutes_the_bits(dtype):
    for nt in (30, 129, switch(dtype), 1000):
        rng = np.random.default_rng(nt)
        x = rng.standard_normal((111, nt)).astype(dtype)
        perm = rng.permutation(111)
        (a,), _ = time_sum([x.reshape(37, 3, nt)])
        (b,), _ = time_sum([x[perm].reshape(37, 3, nt)])
        (c,), _ = time_sum([x[perm].reshape(111, 1, nt)])
        (d,), _ = time_sum([x[perm].reshape(1, 111, nt)])
        assert a.reshape(-1)[perm].tobytes() == b.tobytes() == c.tobytes() == d.tobytes(), nt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_time_sum_accumulates_blocks_within_the_bound_of_the_whole(dtype):
    x = np.random.default_rng(2).standard_normal((37, 6, 5)).astype(dtype)
    ref, tol = bound(x)
    (whole,), _ = time_sum([x])
    g, parts = None, []
    for t0, t1 in ((0, 2), (2, 4), (4, 5)):
        blk = np.ascontiguousarray(x[..., t0:t1])
        (part,), _ = time_sum([blk])
        before = None if g is None else g.numpy()[0]
        (now,), g = time_sum([blk], accumulate_into=g)
        # += with one further rounding: exactly the earlier accumulator plus the block's own sum
        assert now.tobytes() == (part if before is None else before + part).tobytes()
        parts.append(part)
    assert np.all(np.abs(now - ref) <= tol) and np.all(np.abs(whole - ref) <= tol)


def test_time_sum_refuses_overlap_and_misalignment_on_the_device():
    from pytemdiags_amd import _clim
    lib = _clim.load()
    ncol, nlev, nt = 4, 3, 5
    src = torch.zeros(ncol * nlev * nt + 16, dtype=torch.float64, device=DEV)
    acc = torch.full((64,), CANARY, dtype=torch.float64, device=DEV)

    def call(s, a, dt=0, flags=0, nf=1):
        sp = (C.c_void_p * nf)(*([s] if nf == 1 else s))
        ap = (C.c_void_p * nf)(*([a] if nf == 1 else a))
        return lib.temxc_time_sum(0, nf, sp, (C.c_int * nf)(*([dt] * nf)), ap, ncol, nlev, nt, flags, None)
    assert call(src.data_ptr(), src.data_ptr() + 8 * (ncol * nlev * nt - 1)) == -1 and b"overlaps src" in lib.temx_last_error()
    assert call(src.data_ptr(), src.data_ptr()) == -1
    assert call([src.data_ptr(), src.data_ptr()], [acc.data_ptr(), acc.data_ptr() + 8 * 11], nf=2) == -1
    assert b"overlaps acc" in lib.temx_last_error()
    assert call(src.data_ptr() + 4, acc.data_ptr()) == -1 and b"aligned" in lib.temx_last_error()
    assert call(src.data_ptr(), acc.data_ptr() + 4) == -1 and b"aligned" in lib.temx_last_error()
    assert call(src.data_ptr() + 2, acc.data_ptr(), dt=1) == -1
    assert call(src.data_ptr(), acc.data_ptr(), flags=4) == -1
    torch.cuda.synchronize()
    assert torch.all(acc == CANARY)                                        # a refused call wrote nothing
    assert call(src.data_ptr() + 4, acc.data_ptr() + 8, dt=1) == 0           # fp32 at 4 mod 8, the acc next to the src
    assert call(src.data_ptr(), src.data_ptr() + 8 * ncol * nlev * nt) == 0  # touching, not overlapping
    torch.cuda.synchronize()
    assert torch.all(acc[1:13] == 0) and acc[0] == CANARY and torch.all(acc[13:] == CANARY)


# ---- temxc_tem_from_zonal_means -----------------------------------------------------------------------------------------
def tem_case(nlev=6, nt=5, L=20, ne=4, seed=3, dtype=np.float64):
    key = ("tem", nlev, nt, L, ne, seed, np.dtype(dtype).name)
    if key not in _cache:
        from pytemdiags_amd import synth
        lat, lon = synth.cubed_sphere_gll(ne)[:2]
        plev = synth.pressure_levels(nlev)
        f = [x.astype(dtype) for x in synth.analytic_fields(lat, lon, plev, nt, seed=seed)]
        for x in f:
            x.setflags(write=False)
        _cache[key] = (lat, lon, plev, f)
    return _cache[key]


@pytest.mark.parametrize("nlev,nt,dlat", [(6, 5, 1), (41, 26, 1), (6, 200, 3)])
def test_own_zonal_means_fed_back_reproduce_the_run_bit_for_bit(nlev, nt, dlat):
    """The three shapes take the three variants of the epilogue: the scan inside one workgroup per latitude
    (nlev * nt <= 1024), the wavefront scan in a launch of its own (nlev > 40), the loop per point."""
    from pytemdiags_amd import engine
    lat, lon, plev, f = tem_case(nlev, nt)
    plan = engine.Plan(lat, orc.zm_latitudes(dlat), 20, device=0)
    plan.set_tem(nlev, nt, plev * 100)
    d = [torch.as_tensor(x, device=DEV) for x in f]
    res, zon = plan.tem_run(*d, want_zonal=True)
    assert not plan.status()
    res2, zon2 = plan.tem_from_zonal_means(zon[:7].clone(), want_zonal=True)
    assert torch.equal(res, res2) and torch.equal(zon, zon2)
    res3, none = plan.tem_from_zonal_means(zon[:7].clone())
    assert none is None and torch.equal(res, res3)
    plan.close()


def test_from_zonal_means_matches_the_oracle_and_leaves_the_plan_alone():
    from conftest import fieldnorm_err
    from pytemdiags_amd import engine, synth
    RES, ZON = _names()
    lat, lon, plev, f = tem_case()
    q = synth.analytic_tracer(lat, lon, plev, 5, which=0)
    ref = clim_reference(f, lat, plev, 20, key="ne4x6x5")

    def sequence(call_between):
        plan = engine.Plan(lat, orc.zm_latitudes(1), 20, device=0)
        with pytest.raises(Exception) as ei:                     # before set_tem: TEMX_ESTATE, from the library itself
            from pytemdiags_amd import _clim, _lib
            z = torch.zeros((8, plan.M, 6, 1), dtype=torch.float64, device=DEV)
            r = torch.zeros((10, plan.M, 6, 1), dtype=torch.float64, device=DEV)
            rc = _clim.load().temxc_tem_from_zonal_means(plan._h, C.c_void_p(z.data_ptr()), 1, C.c_void_p(r.data_ptr()),
                                                         None, None)
            assert rc == -5
            _lib.check(rc)
        assert ei.value.code == -5
        with pytest.raises(Exception) as ei:
            plan.tem_from_zonal_means(torch.zeros((7, plan.M, 6, 1), dtype=torch.float64, device=DEV))
        assert ei.value.code == -5
        plan.set_tem(6, 5, plev * 100)
        d = [torch.as_tensor(x, device=DEV) for x in f]
        dq = torch.as_tensor(q, device=DEV)
        res, zon = plan.tem_run(*d, want_zonal=True)
        got = None
        if call_between:                                         # nts = 1 on a plan set for nt = 5
            got = {}
            for name in SETS:
                zm7 = torch.as_tensor(np.stack([ref["zm"][name][n] for n in ZM7]), device=DEV)
                got[name] = plan.tem_from_zonal_means(zm7, want_zonal=True)
        eddy = plan.tem_eddy(*d)
        tres, tzon = plan.tracer_run(dq, d[1], d[3], want_zonal=True)
        assert not plan.status()
        plan.close()
        return res, zon, eddy, tres, tzon, got
    a, b = sequence(False), sequence(True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][n], b[2][n]) for n in a[2])       # tem_eddy and tracer_run: as if it had not been called
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for name in SETS:
        res, zon = (x.cpu().numpy() for x in b[5][name])
        assert res.shape == (10, 180, 6, 1) and zon.shape == (16, 180, 6, 1)
        o = ref["sets"][name]
        for i, n in enumerate(RES):
            e = fieldnorm_err(res[i], getattr(o, n)())
            assert e <= 1e-10, (name, n, e)
        for i, n in enumerate(ZON):
            e = fieldnorm_err(zon[i], getattr(o, n))
            assert e <= 1e-10, (name, n, e)


def test_nan_in_one_latitude_gives_the_nan_pattern_of_the_oracle():
    from pytemdiags_amd import engine
    RES, ZON = _names()
    lat, lon, plev, f = tem_case()
    ref = clim_reference(f, lat, plev, 20, key="ne4x6x5")
    zm = {n: ref["zm"]["total"][n].copy() for n in ZM7}
    for n in ZM7:
        zm[n][77] = np.nan
    with np.errstate(all="ignore"):
        o = orc.TEMOracle.from_zonal_means(zm, ref["full"].plev)
    plan = engine.Plan(lat, orc.zm_latitudes(1), 20, device=0)
    plan.set_tem(6, 5, plev * 100)
    res, zon = (x.cpu().numpy() for x in plan.tem_from_zonal_means(
        torch.as_tensor(np.stack([zm[n] for n in ZM7]), device=DEV), want_zonal=True))
    plan.close()
    some = 0
    for i, n in enumerate(RES):
        want = np.isnan(getattr(o, n)())
        assert np.array_equal(np.isnan(res[i]), want), n
        some += int(want.sum())
        assert 0 < want.sum() < want.size, n
    for i, n in enumerate(ZON):
        assert np.array_equal(np.isnan(zon[i]), np.isnan(getattr(o, n))), n
    assert some


# ---- front end ----------------------------------------------------------------------------------------------------------
def grid(kind):
    from pytemdiags_amd import synth
    if kind == "random":                              # the generator of test_gpu_binned.py::grid("random")
        rng = np.random.default_rng(3)
        n = 3000
        return np.rad2deg(np.arcsin(rng.uniform(-1, 1, n))), rng.uniform(0, 360, n)
    return synth.cubed_sphere_gll(int(kind[2:]))[:2]


def front_case(kind, nt, dtype=np.float64, L=20, nlev=6):
    """(lat, plev, fields, reference) of one front-end case: computed once, shared, left unchanged."""
    key = ("front", kind, nt, np.dtype(dtype).name, L, nlev)
    if key not in _cache:
        from pytemdiags_amd import synth
        lat, lon = grid(kind)
        plev = synth.pressure_levels(nlev)
        f = [x.astype(dtype) for x in synth.analytic_fields(lat, lon, plev, nt, seed=5)]
        for x in f:
            x.setflags(write=False)
        _cache[key] = (lat, plev, f, clim_reference(f, lat, plev, L))
    return _cache[key]


def values(rs):
    RES, ZON = _names()

    def host(x):                                       # results come back as the kind that went in
        return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    out = {n: host(getattr(rs, n)()) for n in RES}
    out.update({n: host(getattr(rs, n)) for n in ZON})
    return out


def oracle_values(o):
    RES, ZON = _names()
    out = {n: np.asarray(getattr(o, n)(), dtype=np.float64) for n in RES}
    out.update({n: np.asarray(getattr(o, n), dtype=np.float64) for n in ZON})
    return out


def compare(got, want, total, tol, tag):
    """``got``, ``want``: {set: {name: array}}; ``total``: the reference's total set, whose maxima normalise the
    transient set and the four linear results of every set."""
    worst = (0.0, "")
    for s in SETS:
        for n, r in want[s].items():
            x = got[s][n]
            assert x.shape == r.shape == (r.shape[0], r.shape[1], 1), (s, n, x.shape, r.shape)
            den = np.max(np.abs(total[n] if (s == "transient" or n in LINEAR) else r))
            e = float(np.max(np.abs(x - r)) / den)
            worst = max(worst, (e, "%s.%s" % (s, n)))
            assert e <= tol, (tag, s, n, e)
    print("%s: worst normalised error %.2e (%s)" % (tag, worst[0], worst[1]))
    return worst[0]


def check_against_oracle(cl, ref, tol, tag):
    want = {"total": oracle_values(ref["sets"]["total"]), "stationary": oracle_values(ref["stat"]),
            "transient": oracle_values(ref["sets"]["transient"])}
    got = {s: values(getattr(cl, s)) for s in SETS}
    compare(got, want, want["total"], tol, tag)
    # stationary + transient = total for the four results that are linear and homogeneous in the fluxes
    for n in LINEAR:
        e = float(np.max(np.abs(got["stationary"][n] + got["transient"][n] - got["total"][n])) / np.max(np.abs(got["total"][n])))
        assert e <= 1e-12, (tag, n, e)
    return got


def build(kind, nt, dtype=np.float64, L=20, **kw):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f, ref = front_case(kind, nt, dtype, L)
    return TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, **kw), ref


@pytest.mark.parametrize("kind,nt,kw", [("cs8", 5, {}), ("random", 5, {}), ("random", 5, {"lat_bins": True}), ("cs4", 1, {}),
                                        ("cs4", 5, {"L": 30})],
                         ids=["cs8-classes", "random-generic", "random-binned", "cs4-nt1", "cs4-L30"])
def test_climatology_matches_the_oracle(kind, nt, kw):
    from pytemdiags_amd import climatology
    tem, ref = build(kind, nt, climatology=True, **kw)
    cl = tem.climatology
    assert isinstance(cl, climatology.TEMClimatology) and cl.nt == nt
    if kind == "random":
        assert tem.sweep_form == ("binned" if kw.get("lat_bins") else "two-pass")
    got = check_against_oracle(cl, ref, 1e-10, "%s nt=%d %s" % (kind, nt, kw))
    assert set(cl.total.results()) == set(_names()[0])
    np.testing.assert_array_equal(cl.total.results()["epfy"], cl.total.epfy())
    np.testing.assert_array_equal(cl.time, [np.mean(np.arange(nt))])
    # the sets share the mean state
    for n in ZM7[:4]:
        assert np.array_equal(got["total"][n], got["stationary"][n]) and np.array_equal(got["total"][n], got["transient"][n])
    if nt == 1:                                                 # one snapshot: the transient part is rounding
        for n in FLUXES:
            assert np.max(np.abs(got["transient"][n])) <= 1e-12 * np.max(np.abs(got["total"][n])), n


def test_climatology_of_fp32_fields():
    tem, ref = build("cs4", 5, np.float32, climatology=True)
    cl = tem.climatology
    assert cl.total.epfy().dtype == np.float32 and cl.total.psi.dtype == np.float64 and cl.transient.vtem().dtype == np.float32
    want = {"total": oracle_values(ref["sets"]["total"]), "stationary": oracle_values(ref["stat"]),
            "transient": oracle_values(ref["sets"]["transient"])}
    compare({s: values(getattr(cl, s)) for s in SETS}, want, want["total"], 2e-5, "cs4 fp32")


def test_labelled_input_gets_labelled_sets_at_the_mean_time():
    from pytemdiags_amd import LabeledArray, TEMDiagnostics
    lat, plev, f, ref = front_case("cs4", 5)
    t = np.array([10.0, 11.0, 12.0, 13.0, 19.0])
    lab = [LabeledArray(x, ("ncol", "plev", "time"), {"plev": plev, "time": t}, name=n)
           for x, n in zip(f, ("ua", "va", "ta", "wap"))]
    tem = TEMDiagnostics(*lab, lat, L=20, debug_level=0, climatology=True)
    raw, _ = build("cs4", 5, climatology=True)
    x = tem.climatology.transient.epdiv()
    assert x.dims == ("lat", "plev", "time") and x.values.shape == (180, 6, 1)
    np.testing.assert_array_equal(tem.climatology.time, [13.0])
    np.testing.assert_array_equal(x.values, raw.climatology.transient.epdiv())
    assert tem.climatology.stationary.ub.dims == ("lat", "plev", "time")


def tensors(cl):
    return {s: (getattr(cl, s)._res.cpu().numpy(), getattr(cl, s)._zon.cpu().numpy()) for s in SETS}


def as_dicts(t):
    RES, ZON = _names()
    out = {}
    for s, (res, zon) in t.items():
        out[s] = {n: res[i] for i, n in enumerate(RES)}
        out[s].update({n: zon[i] for i, n in enumerate(ZON)})
    return out


@pytest.mark.parametrize("source", ["device", "host-time-major"])
def test_blocked_climatology_against_the_whole_run(source):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f, ref = front_case("cs4", 5)
    whole, _ = build("cs4", 5, climatology=True)
    want = as_dicts(tensors(whole.climatology))
    if source == "device":
        args, kw = [torch.as_tensor(x, device=DEV) for x in f], {}
    else:
        args, kw = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in f], {"dims": ("time", "plev", "ncol")}
    kw.update(plev=plev, L=20, debug_level=0, climatology=True)
    two = TEMDiagnostics(*args, lat, time_block=2, **kw)
    assert two.climatology.nt == 5 and two.climatology.time_sum_path == whole.climatology.time_sum_path
    compare(as_dicts(tensors(two.climatology)), want, want["total"], 1e-11, "time_block=2 from %s" % source)
    check_against_oracle(two.climatology, ref, 1e-10, "time_block=2 from %s, oracle" % source)
    with pytest.raises(RuntimeError, match="time_block"):
        two.up
    five = TEMDiagnostics(*args, lat, time_block=5, **kw)
    for s, (res, zon) in tensors(five.climatology).items():
        assert res.tobytes() == tensors(whole.climatology)[s][0].tobytes(), s
        assert zon.tobytes() == tensors(whole.climatology)[s][1].tobytes(), s


def test_per_snapshot_run_and_native_outputs_are_those_of_an_object_without_climatology():
    from pytemdiags_amd import TEMDiagnostics, synth
    RES, ZON = _names()
    lat, plev, f, _ = front_case("cs8", 5)
    lon = grid("cs8")[1]
    q = synth.analytic_tracer(lat, lon, plev, 5, which=0)
    plain = TEMDiagnostics(*f, lat, plev=plev, L=20, debug_level=0, q=q)
    with pytest.raises(RuntimeError, match="climatology=True"):
        plain.climatology
    tem = TEMDiagnostics(*f, lat, plev=plev, L=20, debug_level=0, q=q, climatology=True)
    assert tem.climatology.nt == 5
    assert torch.equal(tem._res, plain._res) and torch.equal(tem._zon, plain._zon)
    for n in RES:
        np.testing.assert_array_equal(getattr(tem, n)(), getattr(plain, n)())
    np.testing.assert_array_equal(tem.etfy(), plain.etfy())
    np.testing.assert_array_equal(tem.up, plain.up)               # the plan's state is that of the ordinary run
    np.testing.assert_array_equal(tem.vptp, plain.vptp)
    np.testing.assert_array_equal(tem.qp[0], plain.qp[0])          # tracer eddies
    np.testing.assert_array_equal(tem.qpvp[0], plain.qpvp[0])
    for (a0, a1, a), (b0, b1, b) in zip(tem.iter_native(chunk_cols=1024), plain.iter_native(chunk_cols=1024)):
        assert (a0, a1) == (b0, b1)
        for n in a:
            np.testing.assert_array_equal(a[n], b[n])


def test_from_model_levels_passes_climatology_through():
    from test_vertical_host import PLEV37, frontend_case, hybrid_pressure, inside_everywhere
    from pytemdiags_amd import TEMDiagnostics, interp_to_pressure
    lat, lon, hyam, hybm, ps, f = frontend_case()
    levels = PLEV37[inside_everywhere(hybrid_pressure(hyam, hybm, ps), PLEV37 * 100.0)]
    kw = dict(L=30, debug_level=0, climatology=True)
    a = TEMDiagnostics.from_model_levels(*f, lat, plev=levels, ps=ps, hyam=hyam, hybm=hybm, **kw)
    g = interp_to_pressure(f, levels, ps=ps, hyam=hyam, hybm=hybm)
    b = TEMDiagnostics(*g, lat, plev=levels, **kw)
    assert a.climatology.nt == b.climatology.nt == 2
    ta, tb = tensors(a.climatology), tensors(b.climatology)
    for s in SETS:
        assert ta[s][0].tobytes() == tb[s][0].tobytes() and ta[s][1].tobytes() == tb[s][1].tobytes(), s
    np.testing.assert_array_equal(a.up, b.up)
    # time-major model levels, fed by a block source: the fields are kept, so is the plan's state
    tm = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in f]
    c = TEMDiagnostics.from_model_levels(*tm, lat, plev=levels, ps=np.ascontiguousarray(ps.T), hyam=hyam, hybm=hybm,
                                         dims=("time", "lev", "ncol"), **kw)
    plain = TEMDiagnostics.from_model_levels(*tm, lat, plev=levels, ps=np.ascontiguousarray(ps.T), hyam=hyam, hybm=hybm,
                                             dims=("time", "lev", "ncol"), L=30, debug_level=0)
    assert c.climatology.nt == 2
    np.testing.assert_array_equal(c.up, plain.up)
    np.testing.assert_array_equal(c.vtem(), plain.vtem())
    want = as_dicts(tb)
    compare(as_dicts(tensors(c.climatology)), want, want["total"], 1e-10, "time-major model levels")


# One unit in the last place (2^-53 relative, a random sign per point) on the time-mean fields moves the stationary set of
# the NUMPY ORACLE by this much of a quantity's maximum, worst quantity (psi and its derivatives), L = 20, 6 levels, nt = 5:
# the stationary eddies are differences of the time-mean fields from their zonal means.
# Regenerate with ``python tools/clim_sensitivity.py`` (CPU only; the figures below are its output rounded up).
ORACLE_SHIFT_PER_ULP = {"cs4": 1.2e-12, "cs8": 3.7e-12, "random": 5.2e-14}


@pytest.mark.parametrize("kind", ["random", "cs4", "cs8"])
def test_time_sum_path_follows_the_gate_and_the_two_paths_agree(kind, monkeypatch):
    """The two paths differ by the order of their fp64 additions.  Each sum is within (nt - 1) 2^-53 sum|x| of the exact
    one, so the two time means differ by at most 2 (nt - 1) = 8 units in the last place at nt = 5.  What that does to the
    results is a property of the data, measured on the reference alone (ORACLE_SHIFT_PER_ULP).  The 1e-12 the check is
    set at holds where the reference itself is conditioned for it, the 3000 random latitudes (8 x 5.2e-14 = 4e-13); on
    the class grids the bound is 8 units times the reference's shift per unit, 1e-11 on cs4 and 3e-11 on cs8 (measured
    on cs4 for the record: 1.15e-12, stationary ``psi``)."""
    from pytemdiags_amd import climatology
    tol = {"random": 1e-12, "cs4": 8 * ORACLE_SHIFT_PER_ULP["cs4"], "cs8": 8 * ORACLE_SHIFT_PER_ULP["cs8"]}[kind]
    assert 8 * ORACLE_SHIFT_PER_ULP["random"] <= 1e-12
    tem, _ = build(kind, 5, climatology=True)
    assert tem.climatology.time_sum_path == ("kernel" if climatology.TIME_SUM_KERNEL["float64"] else "torch")
    tem32, _ = build("cs4", 5, np.float32, climatology=True)
    assert tem32.climatology.time_sum_path == ("kernel" if climatology.TIME_SUM_KERNEL["float32"] else "torch")
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(climatology, "TIME_SUM_KERNEL", {"float64": on, "float32": on})
        t, _ = build(kind, 5, climatology=True)
        assert t.climatology.time_sum_path == ("kernel" if on else "torch")
        runs[on] = as_dicts(tensors(t.climatology))
    compare(runs[True], runs[False], runs[False]["total"], tol, "kernel path against torch path, %s" % kind)
