"""Time-mean TEM of fields with missing values on the MI355X: the sum over valid times (temxn_time_sum_valid) and
``TEMDiagnostics(..., climatology=True, missing="mask", min_time_coverage=v)``.

Bounds.
  * sums against ``np.sum(np.where(valid, x, 0).astype(float64), -1)``, per row: |delta| <= 2 nt 2^-53 sum_valid |x_t|
    (any order of fp64 additions of at most nt terms is within (nt - 1) 2^-53 sum|x| of the exact sum, so two orders are
    within twice that); counts exact; a row of one valid element bit for bit.  Blocks accumulated against the whole:
    the same bound; against the earlier accumulator plus the block's own sum: bit for bit.
  * front end against the numpy reference (tests/test_nclim_host.py, masked_clim_reference): NaN patterns exactly, with
    nothing left out -- the reference's coverages keep a distance of at least 1e-6 from the threshold, asserted here on
    the reference alone; values on finite points 1e-9 for fp64 and 2e-5 for fp32 fields, the masked mode's bounds at
    L = 20 (test_gpu_missing.tol_of), normalised as test_gpu_clim.compare does it: transient quantities and the four
    flux-linear results of every set by the TOTAL's maximum.  Stationary + transient = total for the four linear
    results: 1e-12 where finite.  NaN-free input against the default ``climatology=True``: 1e-11, the bound of
    test_gpu_missing.test_nan_free_input_equals_default_path.  A blocked run against the whole run: 1e-9; one block:
    bit for bit."""
import ctypes as C

import numpy as np
import pytest

from test_clim_host import LINEAR
from test_gpu_clim import CANARY, NCOLS, NLEVS, Guarded, as_dicts, grid, off_by_one, small_plan, tensors
from test_gpu_missing import tol_of
from test_missing_host import surface_mask
from test_nclim_host import masked_clim_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
SETS = ("total", "stationary", "transient")
THR, TTHR, L = 0.5, 0.5, 20
_cache = {}


def switch(dtype, nf, common):
    from pytemdiags_amd import _nclim
    return _nclim.switch_nt(np.dtype(dtype).itemsize, nf, common)


def nts_of(dtype, nf, common):
    s = switch(dtype, nf, common)
    return sorted({1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 129, s - 1, s, s + 1, 1000})


# ---- temxn_time_sum_valid ---------------------------------------------------------------------------------------------
def holes(rng, x):
    """``x`` [nf][rows][nt] with missing values put in, all kinds in one array.  Rows by index mod 8: 1 all missing (in
    one field, the others whole), 2 all valid, 3 only the first time valid, 4 only the last (the missing times spread
    over the fields), the others about 30 % missing at random under the common mask of the nf fields.  Missing values are
    NaN, +Inf and -Inf."""
    nf, rows, nt = x.shape
    p = 1.0 - 0.7 ** (1.0 / nf)
    bad = rng.random(x.shape) < p
    r = np.arange(rows)
    which = rng.integers(0, nf, (rows, nt))                    # the one field a forced hole goes to
    one = np.arange(nf)[:, None, None] == which[None]
    t = np.arange(nt)[None, :]
    forced = np.zeros((rows, nt), dtype=bool)
    forced |= (r % 8 == 1)[:, None]
    forced |= (r % 8 == 3)[:, None] & (t > 0)
    forced |= (r % 8 == 4)[:, None] & (t < nt - 1)
    keep = np.isin(r % 8, (1, 2, 3, 4))[None, :, None]
    bad = np.where(keep, one & forced[None], bad)
    kinds = np.array([np.nan, np.inf, -np.inf])[rng.integers(0, 3, x.shape)]
    return np.where(bad, kinds, x).astype(x.dtype)


def reference(fields, common):
    """-> (sums [nf][...], counts [nf][...] -- equal under a common mask --, bounds [nf][...])"""
    fin = np.stack([np.isfinite(x) for x in fields])
    valid = np.broadcast_to(fin.all(axis=0), fin.shape) if common else fin
    x64 = np.stack([np.where(v, x, 0).astype(np.float64) for x, v in zip(fields, valid)])
    nt = fields[0].shape[-1]
    return np.sum(x64, -1), valid.sum(-1).astype(np.float64), 2.0 * nt * 2.0 ** -53 * np.sum(np.abs(x64), -1)


class GuardedPair:
    """Sums and counts, each a view one element into a canary-filled buffer of its own."""

    def __init__(self, nf, common, ncol, nlev):
        self.a, self.c = Guarded(nf, ncol, nlev), Guarded(1 if common else nf, ncol, nlev)

    def check(self):
        self.a.check()
        self.c.check()


def sum_valid(fields, common, into=None):
    """-> (sums, counts as numpy lists, the guarded outputs); sources and outputs unaligned, canaries checked."""
    plan = small_plan()
    ncol, nlev, _ = fields[0].shape
    g = into or GuardedPair(len(fields), common, ncol, nlev)
    acc, cnt = plan.time_sum_valid([off_by_one(x) for x in fields], acc=g.a.acc, cnt=g.c.acc, accumulate=into is not None,
                                   common=common)
    assert all(o is a for o, a in zip(acc, g.a.acc))
    assert (cnt is g.c.acc[0]) if common else all(o is a for o, a in zip(cnt, g.c.acc))
    torch.cuda.synchronize()
    g.check()
    return g.a.numpy(), g.c.numpy(), g


def check_rows(fields, got, cnt, common, tag):
    """The bounds of one call; -> worst |delta| / bound."""
    ref, rcnt, tol = reference(fields, common)
    worst = 0.0
    for f, x in enumerate(fields):
        c = cnt[0] if common else cnt[f]
        assert got[f].shape == x.shape[:2] and got[f].dtype == np.float64 and c.dtype == np.float64
        assert np.all(np.isfinite(got[f])), (tag, f)                       # a non-finite value never reaches acc
        assert np.array_equal(c, rcnt[f]), (tag, f)                        # counts are exact
        assert np.all(np.abs(got[f] - ref[f]) <= tol[f]), (tag, f, float(np.max(np.abs(got[f] - ref[f]) - tol[f])))
        empty = rcnt[f] == 0
        assert np.all(got[f][empty] == 0) and np.all(c[empty] == 0), (tag, f)
        single = rcnt[f] == 1                                              # one valid element: bitwise that element
        assert got[f][single].tobytes() == ref[f][single].tobytes(), (tag, f)
        worst = max(worst, float(np.max(np.abs(got[f] - ref[f]) / np.maximum(tol[f], 1e-300))))
    return worst


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nf,common", [(1, False), (4, True)], ids=["own-1", "common-4"])
def test_sums_and_counts_every_shape_unaligned_with_canaries(dtype, nf, common):
    rng = np.random.default_rng(11)
    rmax = NCOLS[-1] * NLEVS[-1]
    worst, seen = 0.0, set()
    for nt in nts_of(dtype, nf, common):
        scale = 10.0 ** rng.integers(-3, 4, (nf, rmax, 1))
        big = holes(rng, (rng.standard_normal((nf, rmax, nt)) * scale).astype(dtype))
        small = {}
        for ncol in NCOLS:
            for nlev in NLEVS:
                rows = ncol * nlev
                fields = [big[f, :rows].reshape(ncol, nlev, nt) for f in range(nf)]
                got, cnt, _ = sum_valid(fields, common)
                tag = (np.dtype(dtype).name, nf, common, nt, ncol, nlev)
                worst = max(worst, check_rows(fields, got, cnt, common, tag))
                again, cagain, _ = sum_valid(fields, common)             # repeated calls: identical bits
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got + cnt, again + cagain)), tag
                # equal rows give equal bits whatever ncol, nlev and the row's position: the rows of the largest case
                if rows == rmax:
                    for (c, k), (sa, sc) in small.items():
                        for a, b in zip(sa + sc, got + cnt):
                            assert a.reshape(-1).tobytes() == b.reshape(-1)[:c * k].tobytes(), (tag, c, k)
                else:
                    small[(ncol, nlev)] = (got, cnt)
                seen |= {int(v) for v in np.unique(cnt[0])}
    assert 0 in seen and 1 in seen and 1000 in seen                     # all missing, one valid, all valid occurred
    print("%s nf=%d common=%s: worst |delta| / bound %.3f over nt in %s" % (np.dtype(dtype).name, nf, common, worst,
                                                                           nts_of(dtype, nf, common)))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_eight_fields_common_mask_and_a_field_alone_among_eight(dtype):
    """nf = 8 takes the eight-field instantiation of the common-mask kernels; in own-mask mode the sum of a field does
    not depend on what else the call carries."""
    rng = np.random.default_rng(8)
    for nt in sorted({5, 31, switch(dtype, 8, True) - 1, switch(dtype, 8, True), switch(dtype, 1, False), 700}):
        x = holes(rng, rng.standard_normal((8, 37 * 3, nt)).astype(dtype))
        fields = [x[f].reshape(37, 3, nt) for f in range(8)]
        for nf in (5, 8):
            got, cnt, _ = sum_valid(fields[:nf], True)
            check_rows(fields[:nf], got, cnt, True, ("common", nf, nt))
        own = holes(rng, rng.standard_normal((1, 8 * 37 * 3, nt)).astype(dtype))[0]     # every field its own holes
        fields = [own[f * 111:(f + 1) * 111].reshape(37, 3, nt) for f in range(8)]
        got, cnt, _ = sum_valid(fields, False)
        check_rows(fields, got, cnt, False, ("own", 8, nt))
        for f in (0, 5, 7):
            (alone,), (calone,), _ = sum_valid([fields[f]], False)
            assert alone.tobytes() == got[f].tobytes() and calone.tobytes() == cnt[f].tobytes(), (nt, f)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_time_missing_in_one_of_four_fields_drops_from_all_four_and_the_count(dtype):
    for nt in (7, switch(dtype, 4, True) + 3):
        rng = np.random.default_rng(nt)
        fields = [rng.standard_normal((5, 2, nt)).astype(dtype) for _ in range(4)]
        t = nt // 2
        fields[2][3, 1, t] = np.nan
        fields[0][4, 0, 0] = np.inf
        fields[3][4, 0, nt - 1] = -np.inf
        got, (cnt,), _ = sum_valid(fields, True)
        want = np.full((5, 2), float(nt))
        want[3, 1], want[4, 0] = nt - 1, nt - 2
        assert np.array_equal(cnt, want)
        for f in range(4):
            without = np.delete(fields[f][3, 1].astype(np.float64), t).sum()
            assert abs(got[f][3, 1] - without) <= 2 * nt * 2.0 ** -53 * np.abs(fields[f][3, 1][np.isfinite(fields[f][3, 1])]).sum()
            inner = fields[f][4, 0, 1:nt - 1].astype(np.float64)
            assert abs(got[f][4, 0] - inner.sum()) <= 2 * nt * 2.0 ** -53 * np.abs(inner).sum()
        # own masks: the other three fields keep that time
        own, cown, _ = sum_valid(fields, False)
        assert cown[2][3, 1] == nt - 1 and all(cown[f][3, 1] == nt for f in (0, 1, 3))
        assert cown[0][4, 0] == nt - 1 and cown[3][4, 0] == nt - 1 and cown[1][4, 0] == nt


def test_one_valid_element_is_bitwise_and_keeps_signed_zero_and_subnormals():
    vals = np.array([-0.0, 0.0, 5e-324, -1.5, np.float64(np.float32(1e-45))])
    for nt, pos in ((1, 0), (6, 0), (6, 5), (6, 2), (300, 299)):
        x = np.full((1, 5, nt), np.nan)
        x[0, :, pos] = vals
        for common in (False, True):
            (got,), (cnt,), _ = sum_valid([x], common)
            assert got.tobytes() == vals.reshape(1, 5).tobytes() and np.all(cnt == 1), (nt, pos, common)
        x32 = np.full((3, 1, nt), np.inf, dtype=np.float32)
        v32 = np.array([-0.0, 1e-45, 3.25], dtype=np.float32)
        x32[:, 0, pos] = v32
        (got,), (cnt,), _ = sum_valid([x32], False)
        assert got.tobytes() == v32.astype(np.float64).reshape(3, 1).tobytes() and np.all(cnt == 1)
        both, (cnt,), _ = sum_valid([x32, np.where(np.isfinite(x32), np.float32(2.0), x32)], True)
        assert both[0].tobytes() == got.tobytes() and np.all(both[1] == 2.0) and np.all(cnt == 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("common", [False, True], ids=["own", "common"])
def test_permuting_rows_permutes_the_bits(dtype, common):
    nf = 4 if common else 1
    for nt in (30, 129, switch(dtype, nf, common), 1000):
        rng = np.random.default_rng(nt)
        x = holes(rng, rng.standard_normal((nf, 111, nt)).astype(dtype))
        perm = rng.permutation(111)

        def run(rows, shape):
            got, cnt, _ = sum_valid([rows[f].reshape(shape + (nt,)) for f in range(nf)], common)
            return [v.reshape(-1) for v in got + cnt]
        a = run(x, (37, 3))
        for shape in ((37, 3), (111, 1), (1, 111)):
            b = run(x[:, perm], shape)
            assert all(u[perm].tobytes() == v.tobytes() for u, v in zip(a, b)), (nt, shape)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("common", [False, True], ids=["own", "common"])
def test_blocks_accumulate_bit_for_bit_and_within_the_bound_of_the_whole(dtype, common):
    nf = 4 if common else 2
    x = holes(np.random.default_rng(2), np.random.default_rng(3).standard_normal((nf, 37 * 6, 5)).astype(dtype))
    fields = [x[f].reshape(37, 6, 5) for f in range(nf)]
    g, now, cnow = None, None, None
    for t0, t1 in ((0, 2), (2, 4), (4, 5)):
        blk = [np.ascontiguousarray(v[..., t0:t1]) for v in fields]
        part, cpart, _ = sum_valid(blk, common)
        before = None if g is None else (g.a.numpy(), g.c.numpy())
        now, cnow, g = sum_valid(blk, common, into=g)
        # += with one further rounding: exactly the earlier accumulator plus the block's own sum; counts add exactly
        for f in range(nf):
            assert now[f].tobytes() == (part[f] if before is None else before[0][f] + part[f]).tobytes(), (t0, f)
        for f in range(len(cnow)):
            assert cnow[f].tobytes() == (cpart[f] if before is None else before[1][f] + cpart[f]).tobytes(), (t0, f)
    check_rows(fields, now, cnow, common, "accumulated")
    whole, cwhole, _ = sum_valid(fields, common)
    check_rows(fields, whole, cwhole, common, "whole")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(cnow, cwhole))


def test_refuses_overlap_and_misalignment_on_the_device_and_writes_nothing():
    from pytemdiags_amd import _nclim
    lib = _nclim.load()
    ncol, nlev, nt = 4, 3, 5
    n = ncol * nlev * nt
    src = torch.zeros(n + 16, dtype=torch.float64, device=DEV)
    out = torch.full((64,), CANARY, dtype=torch.float64, device=DEV)
    P = C.c_void_p

    def call(s, a, c, dt=0, flags=0, nf=1):
        one = lambda v: (P * nf)(*([v] if nf == 1 else v))           # noqa: E731
        return lib.temxn_time_sum_valid(0, nf, one(s), dt, one(a), one(c), ncol, nlev, nt, flags, None)

    def err():
        return lib.temx_last_error()
    s0, o0 = src.data_ptr(), out.data_ptr()
    assert call(s0, s0 + 8 * (n - 1), o0) == -1 and b"acc 0 overlaps src 0" in err()
    assert call(s0, o0, s0 + 8 * (n - 1)) == -1 and b"cnt 0 overlaps src 0" in err()
    assert call(s0, s0, o0) == -1 and call(s0, o0, s0) == -1
    assert call(s0, o0, o0 + 8 * 11) == -1 and b"cnt 0 overlaps acc 0" in err()
    assert call(s0, o0, o0) == -1
    assert call([s0, s0], [o0, o0 + 8 * 11], [o0 + 8 * 24, o0 + 8 * 36], nf=2) == -1 and b"acc 1 overlaps acc 0" in err()
    assert call([s0, s0], [o0, o0 + 8 * 12], [o0 + 8 * 24, o0 + 8 * 35], nf=2) == -1 and b"cnt 1 overlaps cnt 0" in err()
    assert call(s0 + 4, o0, o0 + 8 * 12) == -1 and b"aligned" in err()
    assert call(s0, o0 + 4, o0 + 8 * 12) == -1 and b"aligned" in err()
    assert call(s0, o0, o0 + 8 * 12 + 4) == -1 and b"aligned" in err()
    assert call(s0 + 2, o0, o0 + 8 * 12, dt=1) == -1
    assert call(s0, o0, o0 + 8 * 12, flags=4) == -1 and call(s0, o0, o0 + 8 * 12, dt=3) == -1
    torch.cuda.synchronize()
    assert torch.all(out == CANARY)                                        # a refused call wrote nothing
    # fp32 at 4 mod 8; acc next to the src, cnt next to the acc (touching, not overlapping); cnt[1] unused under a common mask
    assert call(s0 + 4, o0 + 8, o0 + 8 * 13, dt=1) == 0
    assert call([s0, s0 + 8 * n // 2], [o0 + 8 * 26, o0 + 8 * 38], [o0 + 8 * 50, None], dt=1, nf=2, flags=_nclim.COMMON_MASK) == 0
    torch.cuda.synchronize()
    assert torch.all(out[1:13] == 0) and torch.all(out[13:25] == nt) and out[0] == CANARY and out[25] == CANARY
    assert torch.all(out[26:50] == 0) and torch.all(out[50:62] == nt) and torch.all(out[62:] == CANARY)


# ---- front end --------------------------------------------------------------------------------------------------------
def fields_of(kind, dtype=np.float64, nan_free=False):
    """test_gpu_missing.masked_fields' recipe on the grids of test_gpu_clim: ``surface_mask``, its ``plev``, seed 1,
    nlev = 8, nt = 5.  -> (lat, plev, fields, reference or None); computed once, shared, left unchanged."""
    key = ("fields", kind, np.dtype(dtype).name, nan_free)
    if key not in _cache:
        from pytemdiags_amd import synth
        lat, lon = grid(kind)
        nlev, nt = 8, 5
        plev = np.sort(synth.pressure_levels(nlev) * 0.5 + 500.0 * np.linspace(0, 1, nlev) ** 2)
        f = [x.astype(dtype) for x in synth.analytic_fields(lat, lon, plev, nt, seed=1)]
        ref = None
        if not nan_free:
            miss = surface_mask(lat, lon, plev, nt)
            f = [np.where(miss, np.nan, x).astype(dtype) for x in f]
            ref = masked_clim_reference(f, lat, plev, L, THR, TTHR)
        for x in f:
            x.setflags(write=False)
        _cache[key] = (lat, plev, f, ref)
    return _cache[key]


def build(kind, dtype=np.float64, fields=None, **kw):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f, ref = fields_of(kind, dtype)
    kw.setdefault("min_time_coverage", TTHR)
    return TEMDiagnostics(*(f if fields is None else fields), lat, plev=plev, L=L, debug_level=0, climatology=True,
                          missing="mask", min_coverage=THR, **kw), ref


def host(x):
    return np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)


def compare_finite(got, want, total, tol, tag):
    """test_gpu_clim.compare on the points where the reference is finite: ``got``, ``want`` {set: {name: array}};
    ``total`` the reference's total set, whose maxima normalise the transient set and the four linear results."""
    worst = (0.0, "")
    for s in SETS:
        for n, r in want[s].items():
            x = got[s][n]
            assert x.shape == r.shape == (r.shape[0], r.shape[1], 1), (s, n, x.shape, r.shape)
            fin = np.isfinite(r) & np.isfinite(x)
            base = total[n] if (s == "transient" or n in LINEAR) else r
            den = np.max(np.abs(base[np.isfinite(base)]))
            e = float(np.max(np.abs(x[fin] - r[fin])) / den)
            worst = max(worst, (e, "%s.%s" % (s, n)))
            assert e <= tol, (tag, s, n, e)
    print("%s: worst normalised error %.2e (%s)" % (tag, worst[0], worst[1]))
    return worst[0]


MARGINS = {   # the issue's tables: (partial, kept, dropped) on the native grid; (partial, dropped, all NaN, total) on the zonal grid
    "cs4": ((751, 361, 390), (86, 72, 33, 1440)),
    "random": ((2525, 1241, 1284), (129, 78, 28, 1440)),
}


@pytest.mark.parametrize("kind", ["cs4", "random"])
def test_reference_exercises_the_counts_and_keeps_its_margins(kind):
    """On the CPU, on the reference alone: the kernel's counts and the threshold are both exercised, on the native and on
    the zonal grid, and no coverage lies within 1e-6 of the threshold, so NaN patterns can be compared exactly."""
    _, _, f, ref = fields_of(kind)
    nt = f[0].shape[-1]
    c, z, need = ref["count"], ref["zcount"], ref["need"]
    assert need == 3
    part = (c > 0) & (c < nt)
    assert (int(part.sum()), int((part & (c >= need)).sum()), int((part & (c < need)).sum())) == MARGINS[kind][0]
    zp = (z > 0) & (z < nt)
    assert (int(zp.sum()), int((zp & (z < need)).sum()), int((z == 0).sum()), z.size) == MARGINS[kind][1]
    d_snap = float(np.abs(ref["full"].coverage - THR).min())
    d_stat = float(np.abs(ref["stat"].coverage - THR).min())
    print("%s: smallest distance of a coverage from %.1f: per snapshot %.2e, stationary %.2e" % (kind, THR, d_snap, d_stat))
    assert d_snap >= 1e-6 and d_stat >= 1e-6


@pytest.mark.parametrize("kind,dtype", [("cs4", np.float64), ("random", np.float64), ("cs4", np.float32)],
                         ids=["cs4-f64", "random-f64", "cs4-f32"])
def test_masked_climatology_matches_the_reference(kind, dtype):
    from pytemdiags_amd import climatology
    tem, ref = build(kind, dtype)
    cl = tem.climatology
    assert isinstance(cl, climatology.TEMClimatology) and cl.nt == 5 and cl.time_sum_path == "kernel"
    assert tem.min_time_coverage == TTHR and tem.sweep_form == "masked"
    tol = tol_of(L, dtype)
    assert np.abs(ref["full"].coverage - THR).min() >= 1e-6 and np.abs(ref["stat"].coverage - THR).min() >= 1e-6
    # coverages: counts are exact, the zonal coverage of the stationary run is within the masked mode's bound
    tc, sc = host(cl.time_coverage), host(cl.stationary_coverage)
    assert tc.shape == sc.shape == (180, 8, 1)
    assert np.array_equal(tc, ref["time_coverage"])
    assert np.array_equal(np.isnan(sc), np.isnan(ref["stat"].coverage))
    assert np.max(np.abs(sc - ref["stat"].coverage)) <= tol
    # NaN patterns: exactly the reference's, nothing left out
    got = as_dicts(tensors(cl))
    want = ref["values"]
    nans = 0
    for s in SETS:
        assert set(got[s]) == set(want[s]) and len(want[s]) == 26
        for n, r in want[s].items():
            assert np.array_equal(np.isnan(got[s][n]), np.isnan(r)), (s, n, int((np.isnan(got[s][n]) != np.isnan(r)).sum()))
            assert not np.isinf(got[s][n]).any(), (s, n)
            nans += int(np.isnan(r).sum())
    assert nans
    compare_finite(got, want, want["total"], tol, "%s %s" % (kind, np.dtype(dtype).name))
    # stationary + transient = total for the four results that are linear and homogeneous in the fluxes, where finite
    for n in LINEAR:
        S, T, tot = got["stationary"][n], got["transient"][n], got["total"][n]
        fin = np.isfinite(S) & np.isfinite(T) & np.isfinite(tot)
        assert fin.any()
        e = float(np.max(np.abs(S + T - tot)[fin]) / np.max(np.abs(tot[fin])))
        assert e <= 1e-12, (n, e)
    # the sets share the mean state; the getters serve the sets as the unmasked climatology does
    for n in ("ub", "vb", "thetab", "wapb"):
        assert np.array_equal(got["total"][n], got["stationary"][n], equal_nan=True)
        assert np.array_equal(got["total"][n], got["transient"][n], equal_nan=True)
    np.testing.assert_array_equal(cl.total.results()["epfy"], cl.total.epfy())
    assert cl.total.epfy().dtype == dtype and cl.time_coverage.dtype == np.float64


def test_nan_free_input_with_the_new_keywords_equals_the_default_climatology():
    from pytemdiags_amd import TEMDiagnostics
    for kind in ("cs4", "random"):
        lat, plev, f, _ = fields_of(kind, nan_free=True)
        plain = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, climatology=True)
        tem, _ = build(kind, fields=f)
        want, got = as_dicts(tensors(plain.climatology)), as_dicts(tensors(tem.climatology))
        assert all(np.all(np.isfinite(v)) for s in SETS for v in got[s].values())
        compare_finite(got, want, want["total"], 1e-11, "NaN-free %s against the default climatology" % kind)
        assert np.all(host(tem.climatology.time_coverage) == 1.0)
        assert np.max(np.abs(host(tem.climatology.stationary_coverage) - 1.0)) <= 1e-11


@pytest.mark.parametrize("source", ["device", "host-time-major"])
def test_blocked_masked_climatology_against_the_whole_run(source):
    """The surface mask varies per snapshot, so the counts cross block boundaries."""
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f, ref = fields_of("cs4")
    whole, _ = build("cs4")
    want = as_dicts(tensors(whole.climatology))
    if source == "device":
        args, kw = [torch.as_tensor(x, device=DEV) for x in f], {}
    else:
        args, kw = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in f], {"dims": ("time", "plev", "ncol")}
    kw.update(plev=plev, L=L, debug_level=0, climatology=True, missing="mask", min_coverage=THR, min_time_coverage=TTHR)
    two = TEMDiagnostics(*args, lat, time_block=2, **kw)
    assert two.climatology.nt == 5
    got = as_dicts(tensors(two.climatology))
    for s in SETS:
        for n in want[s]:
            assert np.array_equal(np.isnan(got[s][n]), np.isnan(want[s][n])), (s, n)
    compare_finite(got, want, want["total"], 1e-9, "time_block=2 from %s" % source)
    assert np.array_equal(host(two.climatology.time_coverage), ref["time_coverage"])
    five = TEMDiagnostics(*args, lat, time_block=5, **kw)
    for s, (res, zon) in tensors(five.climatology).items():
        assert res.tobytes() == tensors(whole.climatology)[s][0].tobytes(), s
        assert zon.tobytes() == tensors(whole.climatology)[s][1].tobytes(), s
    assert host(five.climatology.stationary_coverage).tobytes() == host(whole.climatology.stationary_coverage).tobytes()


def test_per_snapshot_object_is_that_of_a_masked_run_without_climatology():
    from pytemdiags_amd import TEMDiagnostics, _lib
    lat, plev, f, _ = fields_of("cs4")
    plain = TEMDiagnostics(*f, lat, plev=plev, L=L, debug_level=0, missing="mask", min_coverage=THR)
    tem, _ = build("cs4")
    assert tem.climatology.nt == 5
    assert tem._res.cpu().numpy().tobytes() == plain._res.cpu().numpy().tobytes()
    assert tem._zon.cpu().numpy().tobytes() == plain._zon.cpu().numpy().tobytes()
    np.testing.assert_array_equal(tem.coverage, plain.coverage)
    for n in _lib.RESULT_NAMES:
        np.testing.assert_array_equal(getattr(tem, n)(), getattr(plain, n)())
    np.testing.assert_array_equal(tem.up, plain.up)               # the plan's state is that of the ordinary run
    np.testing.assert_array_equal(tem.vptp, plain.vptp)
    for (a0, a1, a), (b0, b1, b) in zip(tem.iter_native(chunk_cols=512), plain.iter_native(chunk_cols=512)):
        assert (a0, a1) == (b0, b1)
        for n in a:
            np.testing.assert_array_equal(a[n], b[n])
    with pytest.raises(RuntimeError, match="climatology=True"):
        plain.climatology


def test_from_model_levels_passes_the_three_keywords_through():
    """The target levels reach below the surface, so the NaN arise from the remap itself."""
    from test_vertical_host import PLEV37, frontend_case, hybrid_pressure
    from pytemdiags_amd import TEMDiagnostics, interp_to_pressure
    lat, lon, hyam, hybm, ps, f = frontend_case(nt=3)
    p = hybrid_pressure(hyam, hybm, ps)
    levels = PLEV37[(PLEV37 * 100.0 >= p[:, 0, :].max()) & (PLEV37 >= 100.0)]
    below = levels[None, :, None] * 100.0 > ps[:, None, :]                               # targets below the surface
    assert (below.any(axis=-1) & ~below.all(axis=-1)).any()                            # ... at some times and not at others
    kw = dict(L=L, debug_level=0, climatology=True, missing="mask", min_coverage=THR, min_time_coverage=TTHR)
    a = TEMDiagnostics.from_model_levels(*f, lat, plev=levels, ps=ps, hyam=hyam, hybm=hybm, **kw)
    g = interp_to_pressure(f, levels, ps=ps, hyam=hyam, hybm=hybm)
    assert np.isnan(g[0]).any() and not np.isnan(g[0]).all()
    b = TEMDiagnostics(*g, lat, plev=levels, **kw)
    assert a.climatology.nt == b.climatology.nt == 3 and a.min_time_coverage == TTHR
    ta, tb = tensors(a.climatology), tensors(b.climatology)
    for s in SETS:
        assert ta[s][0].tobytes() == tb[s][0].tobytes() and ta[s][1].tobytes() == tb[s][1].tobytes(), s
    assert host(a.climatology.time_coverage).tobytes() == host(b.climatology.time_coverage).tobytes()
    assert host(a.climatology.stationary_coverage).tobytes() == host(b.climatology.stationary_coverage).tobytes()
    tcov = host(b.climatology.time_coverage)
    assert np.isnan(tb["total"][0]).any() and np.isfinite(tb["total"][0]).any()
    # time-major model levels, fed by a block source
    tm = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in f]
    c = TEMDiagnostics.from_model_levels(*tm, lat, plev=levels, ps=np.ascontiguousarray(ps.T), hyam=hyam, hybm=hybm,
                                         dims=("time", "lev", "ncol"), **kw)
    assert c.climatology.nt == 3
    want, got = as_dicts(tb), as_dicts(tensors(c.climatology))
    for s in SETS:
        for n in want[s]:
            assert np.array_equal(np.isnan(got[s][n]), np.isnan(want[s][n])), (s, n)
    compare_finite(got, want, want["total"], 1e-9, "time-major model levels")
    assert np.array_equal(host(c.climatology.time_coverage), tcov)


def test_full_time_coverage_keeps_only_points_valid_in_every_snapshot(monkeypatch):
    """``min_time_coverage=1.0``: the mean fields, as the stationary run receives them, are NaN exactly where any snapshot
    is missing, and elsewhere the reference's means."""
    from pytemdiags_amd import engine
    lat, plev, f, _ = fields_of("cs4")
    ref = masked_clim_reference(f, lat, plev, L, THR, 1.0)
    assert ref["need"] == 5 and np.abs(ref["stat"].coverage - THR).min() >= 1e-6
    seen = []
    run = engine.Plan.tem_run

    def spy(self, ua, va, ta, wap, **kw):
        if ua.shape[-1] == 1:
            seen.append([x.cpu().numpy() for x in (ua, va, ta, wap)])
        return run(self, ua, va, ta, wap, **kw)
    monkeypatch.setattr(engine.Plan, "tem_run", spy)
    tem, _ = build("cs4", min_time_coverage=1.0)
    assert len(seen) == 1
    any_missing = np.isnan(f[0]).any(axis=-1)
    assert any_missing.any() and not any_missing.all()
    for x, m, src in zip(seen[0], ref["means"], f):
        assert x.shape == m.shape and x.dtype == np.float64
        assert np.array_equal(np.isnan(x[..., 0]), any_missing) and np.array_equal(np.isnan(m[..., 0]), any_missing)
        ok = ~any_missing
        bound = 2 * 5 * 2.0 ** -53 * np.abs(src[ok]).sum(-1) / 5 + 2.0 ** -53 * np.abs(m[..., 0][ok])
        assert np.all(np.abs(x[..., 0][ok] - m[..., 0][ok]) <= bound)
    tc = host(tem.climatology.time_coverage)
    assert np.array_equal(tc, ref["time_coverage"])
    got = as_dicts(tensors(tem.climatology))
    for s in SETS:
        for n, r in ref["values"][s].items():
            assert np.array_equal(np.isnan(got[s][n]), np.isnan(r)), (s, n)
    compare_finite(got, ref["values"], ref["values"]["total"], 1e-9, "min_time_coverage=1.0")
