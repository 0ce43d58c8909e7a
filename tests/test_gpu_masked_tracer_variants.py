"""The masked tracer run (include/temx_mtracer.h, csrc/kernels_mtracer.hpp) where test_gpu_masked_tracers.py does not
reach: every instantiation of miss_tracer_project_kernel<T, TB, 2TB, PD>, (fp64, fp32) x TB in {4, 8, 13, 16}, more
than one d-quad, chunk ranges with several whole groups on the clamp-free path, ranges shorter than the register ring,
and a second trip of the grid-stride loops of the native kernels -- against the numpy MaskedTracerOracle of
test_masked_tracers_host.py and its MaskedOracle (``to.mo``) for the masked TEM run every case starts with, which runs
miss_project_kernel<T, 4, TB, 2TB> at (fp64, TB = 16) and at TB = 4 for the first time as well.

TB follows K = L + 1: 4 (K <= 16), 8 (K <= 32), 13 (K <= 52), 16 (K <= 64); PD, the depth of the register ring, is 2
everywhere but in <double, 16, 32, 1>.  Cases, with the instantiation and the path each is there for:

1. test_every_instantiation_matches_the_oracle: the cap mask (surface mask with an empty polar cap, the tracer's gap)
   on cs8 (N = 3458 = 216 * 16 + 2: a ragged last chunk) x 7 x 3 (D = 21: a ragged d-tile, idle waves in the quad).
     L = 12 f64, f32   <double, 4, 8, 2>, <float, 4, 8, 2>     K = 13
     L = 15 f64        <double, 4, 8, 2>                       K = 16, the upper edge of TB = 4
     L = 20 f32        <float, 8, 16, 2>                       K = 21
     L = 50 f32        <float, 13, 26, 2>                      K = 51
     L = 63 f64        <double, 16, 32, 1>                     K = 64, the only PD = 1 ring
   Everything a run gives -- the tracer's coverage, 6 results, 6 zonal arrays and 3 native fields; of the TEM run the
   coverage, 10 results, 16 zonal arrays and 7 native fields -- within ``tol_of(L, dtype)``, NaN patterns equal, and
   no (lat, time) column of the zonal grid ambiguous (coverage within 1e-9 of the threshold).
2. test_scattered_mask_holds_the_tight_bound_at_large_k: holes scattered over the grid (10 % of the points in all five
   arrays, 35 % more of the tracer where |lat| < 25) instead of the cap, min_coverage = 0.  No latitude band is empty,
   the weighted rows are well conditioned (cond <= 3.4 at L = 63) and H has no O(tau) direction, so the bound is the
   1e-9 (fp64) / 2e-5 (fp32) DESIGN.md states for that, at K = 32, 52 and 64, the upper edges of TB = 8, 13 and 16:
     L = 31 f64 <double, 8, 16, 2>   L = 51 f64 <double, 13, 26, 2>   L = 63 f64 <double, 16, 32, 1>
     L = 63 f32 <float, 16, 32, 2>   L = 15 f32 <float, 4, 8, 2>
   Every output on the zonal grid is finite, the native NaN are exactly the missing points.
3. test_many_quads_long_ranges_and_the_second_trip_of_the_native_loops: cs8 x 26 x 50, D = 1300 = 81 * 16 + 4: 82
   d-tiles in 21 quads, the last d-tile of 4 columns, the last quad with two helper waves that only stage.  On 256 CUs
   choose_split gives 24 ranges of 9 or 10 chunks (test_host_tables.py pins that): three whole groups on the clamp-free
   path at PD = 2, eight at PD = 1.  N * D = 4.5 M elements: more than four trips of the loops of
   miss_tracer_native_kernel and miss_eddy_native_kernel.  Column d holds column perm[d] of the 21-column case of
   part 1; what depends on the column alone (not on its level through theta or the derivatives in p) is compared with
   column perm[d] of that case's oracle, and all copies of a base column must be equal bit for bit: the chunk ranges
   do not depend on d, the MFMA order per output column is fixed, there are no atomics.
     L = 50 f64 <double, 13, 26, 2>   L = 63 f64 <double, 16, 32, 1>   L = 12 f32 <float, 4, 8, 2>
4. test_ranges_shorter_than_the_ring: the cap mask on latlon(18, 2) x 3 x 1 (N = 36: three chunks, the last of 4 rows,
   one range, fewer chunks than 2 PD; D = 3: one partial d-tile, three helper waves) at L = 12 (f64, f32) and L = 7
   (f64), and on latlon(13, 1) at L = 3: a grid of one ragged chunk, cfast < c0.  All TB = 4.  Bound 1e-9 / 2e-5.
5. test_tracer_path_equals_tem_path_on_the_same_fit: q = ua with the fields' own mask, so qb, qpvpb, qpwappb, the
   coverage and qp, qpvp, qpwapp must equal ub, upvpb, upwappb, the coverage and up, upvp, upwapp of the TEM run:
   miss_project_kernel<T, 4> + eddy_kernel KIND = 2 against miss_tracer_project_kernel + KIND = 3.  All eight (T, TB)
   on the scattered mask (L = 15, 31, 51, 63) at 1e-11, the project's figure for two GPU paths computing the same
   well-conditioned fit; the cap mask at L = 20 at 1e-11, at L = 50 and 63 within ``tol_of`` with equal NaN patterns.

Bounds: ``tol_of`` of test_gpu_missing.py, 1e-9 / 2e-5 and 1e-11; none is derived from what the kernels give.
Measured on the MI355X (worst field-normalised error of a case over all its outputs, next to its bound):
  1. cap, cs8 x 7 x 3:     L = 12 f64 5.8e-13 (1e-9), L = 12 f32 6.3e-13 (2e-5), L = 15 f64 2.6e-12 (1e-9),
                           L = 20 f32 7.7e-12 (2e-5), L = 50 f32 3.1e-7 (2e-5), L = 63 f64 2.3e-7 (5e-5)
  2. scattered, cs8:       L = 31 f64 4.9e-12 (1e-9), L = 51 f64 2.0e-12 (1e-9), L = 63 f64 2.5e-11 (1e-9),
                           L = 63 f32 2.6e-11 (2e-5), L = 15 f32 2.3e-12 (2e-5)
  3. tiled, cs8 x 26 x 50: L = 50 f64 6.4e-7 (1e-6), L = 63 f64 3.4e-7 (5e-5), L = 12 f32 1.6e-13 (2e-5); all copies of
                           a base column bitwise equal
  4. latlon(18, 2):        L = 12 f64 2.6e-12 (1e-9), L = 12 f32 2.6e-12 (2e-5), L = 7 f64 2.7e-13 (1e-9);
     latlon(13, 1):        L = 3 f64 2.7e-13 (1e-9).  Plan creation serves both grids: nothing had to be replaced
  5. same fit:             0 in all fourteen cases (bounds 1e-11, and 1e-6 / 2e-5 / 5e-5 on the cap at L = 50, 63): with
                           D = 21 both projections get the same chunk ranges (choose_split picks the same nsplit for
                           one quad whatever the slots), so the two paths sum in the same order
No (lat, time) column is ambiguous in any case; the smallest |coverage - 0.5| of the oracles is 8.5e-7 (cap, L = 20).
A scratch build that re-loads the ring slot of <double, 16, 32, 1> before it is consumed fails the L = 63 fp64 cases
of parts 1, 2, 3 and 5 and nothing else; one whose clamp-free loads are a chunk off from the third whole group of a
range on fails all of part 3 (and the L = 63 fp64 cases, whose ring of one has that many groups in a range of four)
and nothing in test_gpu_masked_tracers.py.
"""
import numpy as np
import pytest

from test_gpu_masked_tracers import TRACER_RESULTS, case, tracer_out
from test_gpu_missing import NATIVE, RESULTS, THR, ZONAL, ambiguous, err, grid, run_plan, same_nans, tol_of
from test_masked_tracers_host import TRACER_NATIVE, TRACER_ZONAL, MaskedTracerOracle, masked_tracer_fields
from test_missing_host import latlon

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F64, F32 = np.float64, np.float32
NLEV, NT = 7, 3                                     # D = 21: the 21 columns of parts 1, 2, 3 (base) and 5
_cache = {}


def tight(dtype):
    """The project's bound where the fit is well conditioned: ``tol_of`` without a CAP_TOL entry."""
    return 1e-9 if dtype == F64 else 2e-5


def scattered_fields(lat, lon, nlev, nt, dtype=F64):
    """The fields and the tracer of ``masked_tracer_fields`` without the surface mask and the tracer's gap; in their
    place a fixed-seed random 10 % of the points missing in all five arrays and a further 35 % in the tracer alone
    where |lat| < 25.  -> (plev, [ua, va, ta, wap], q)"""
    from pytemdiags_amd import synth
    plev = np.sort(synth.pressure_levels(nlev) * 0.5 + 500.0 * np.linspace(0, 1, nlev) ** 2)
    f = list(synth.analytic_fields(lat, lon, plev, nt, seed=1)) + [synth.analytic_tracer(lat, lon, plev, nt)]
    rng = np.random.default_rng(11)
    common = rng.random(f[0].shape) < 0.10
    own = (rng.random(f[0].shape) < 0.35) & (np.abs(np.asarray(lat)) < 25.0)[:, None, None]
    f = [np.where(common, np.nan, x).astype(dtype) for x in f]
    f[4] = np.where(own, np.nan, f[4]).astype(dtype)
    return plev, f[:4], f[4]


def scattered_case(L, dtype):
    """Inputs and oracle (min_coverage = 0) of one scattered-mask shape on cs8, computed once and left unchanged."""
    key = ("scattered", L, np.dtype(dtype).name)
    if key not in _cache:
        lat, lon = grid("cs8")
        plev, f, q = scattered_fields(lat, lon, NLEV, NT, dtype=dtype)
        _cache[key] = (lat, lon, plev, f, q, MaskedTracerOracle(*f, q, lat, plev, L, min_coverage=0.0))
    return _cache[key]


def small_case(nlat, nlon, L, dtype):
    key = ("latlon", nlat, nlon, L, np.dtype(dtype).name)
    if key not in _cache:
        lat, lon = latlon(nlat, nlon)
        plev, f, q = masked_tracer_fields(lat, lon, 3, 1, dtype=dtype)
        _cache[key] = (lat, lon, plev, f, q, MaskedTracerOracle(*f, q, lat, plev, L, min_coverage=THR))
    return _cache[key]


def check_run(label, lat, plev, f, q, to, L, tol, min_coverage=THR):
    """A masked TEM run, the masked tracer run and both sets of native fields against the oracle: values within
    ``tol``, NaN patterns equal, no ambiguous (lat, time) column.  -> (worst error, plan, outputs) for more checks."""
    plan, dev, out = run_plan(lat, plev, f, L, min_coverage=min_coverage)
    qd, tres, tzon, tcov = tracer_out(plan, dev, q)
    assert not plan.status()                                   # non-finite input is data in this mode
    if min_coverage > 0:
        amb = ambiguous(to.coverage) | ambiguous(to.mo.coverage)
    else:                                                      # nothing is thresholded: no pattern can be ambiguous
        amb = np.zeros((to.coverage.shape[0], 1, to.coverage.shape[2]), bool)
    assert not amb.any()
    worst = [0.0]

    def close(name, x, ref, exact_nans=False):
        e = err(x, ref)
        worst[0] = max(worst[0], e)
        assert e <= tol, (label, name, e, tol)
        if exact_nans:
            assert np.array_equal(np.isnan(x), np.isnan(ref)), (label, name)
        else:
            assert same_nans(x, ref, amb) == 0, (label, name)
    # the tracer run
    close("tracer coverage", tcov, to.coverage)
    for i, n in enumerate(TRACER_RESULTS):
        close(n, tres[i], to.results[n])
    for i, n in enumerate(TRACER_ZONAL):
        close(n, tzon[i], to.zonal[n])
    eddy = plan.tracer_eddy_masked(qd, dev[1], dev[3])
    tnat = {n: eddy[n].cpu().numpy() for n in TRACER_NATIVE}
    for n in TRACER_NATIVE:
        close(n, tnat[n], to.native[n], exact_nans=True)
    # the TEM run before it
    close("coverage", out["cov"], to.mo.coverage)
    assert np.array_equal(plan.coverage().cpu().numpy().reshape(out["cov"].shape), out["cov"])   # the tracer run left it
    for i, n in enumerate(RESULTS):
        close(n, out["res"][i], to.mo.results[n])
    for i, n in enumerate(ZONAL):
        close(n, out["zon"][i], to.mo.zonal[n])
    eddy = plan.tem_eddy(*dev)
    nat = {n: eddy[n].cpu().numpy() for n in NATIVE}
    for n in NATIVE:
        close(n, nat[n], to.mo.native[n], exact_nans=True)
    print("%s: worst error %.2e (bound %.1e)" % (label, worst[0], tol))
    return worst[0], plan, dict(out, tres=tres, tzon=tzon, tcov=tcov, tnat=tnat, nat=nat)


# ---- 1. every instantiation, against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("L,dtype", [(12, F64), (12, F32), (15, F64), (20, F32), (50, F32), (63, F64)])
def test_every_instantiation_matches_the_oracle(L, dtype):
    lat, lon, plev, f, q, to = case("cs8", L, NLEV, NT, dtype)
    label = "cap cs8 L=%d %s" % (L, np.dtype(dtype).name)
    _, plan, o = check_run(label, lat, plev, f, q, to, L, tol_of(L, dtype))
    assert np.isnan(o["tzon"][0]).any() and np.isfinite(o["tzon"][0]).any()
    assert np.any(o["tcov"] < o["cov"] - 0.05)                 # the tracer's gap costs coverage the TEM run keeps


# ---- 2. a well-conditioned mask: large K held to the tight bound ----------------------------------------------------
@pytest.mark.parametrize("L,dtype", [(31, F64), (51, F64), (63, F64), (63, F32), (15, F32)])
def test_scattered_mask_holds_the_tight_bound_at_large_k(L, dtype):
    lat, lon, plev, f, q, to = scattered_case(L, dtype)
    label = "scattered cs8 L=%d %s" % (L, np.dtype(dtype).name)
    _, plan, o = check_run(label, lat, plev, f, q, to, L, tight(dtype), min_coverage=0.0)
    for n in ("res", "zon", "cov", "tres", "tzon", "tcov"):
        assert np.all(np.isfinite(o[n])), n
    common = ~np.all(np.isfinite(np.stack(f)), axis=0)
    own = common | ~np.isfinite(q)
    assert own.sum() > common.sum() > 0
    for n in TRACER_NATIVE:
        assert np.array_equal(np.isnan(o["tnat"][n]), own), n
    for n in NATIVE:
        assert np.array_equal(np.isnan(o["nat"][n]), common), n


# ---- 3. more than one quad, long ranges, a second trip of the native loops ------------------------------------------
BIG_NLEV, BIG_NT = 26, 50                           # D = 1300 = 81 * 16 + 4
TEM_ZONAL_BY_COLUMN = ("ub", "vb", "wapb", "upvpb", "upwappb")      # not thetab, vptpb: theta carries the level
TEM_NATIVE_BY_COLUMN = ("up", "vp", "wapp", "upvp", "upwapp")


@pytest.mark.parametrize("L,dtype", [(50, F64), (63, F64), (12, F32)])
def test_many_quads_long_ranges_and_the_second_trip_of_the_native_loops(L, dtype):
    lat, lon, plev, f, q, to = case("cs8", L, NLEV, NT, dtype)
    assert not (ambiguous(to.coverage) | ambiguous(to.mo.coverage)).any()
    N, D0, D = lat.size, NLEV * NT, BIG_NLEV * BIG_NT
    rng = np.random.default_rng(5)
    perm = rng.permutation(np.concatenate([np.arange(D0), rng.integers(0, D0, D - D0)]))
    assert np.array_equal(np.unique(perm), np.arange(D0))
    first = np.array([np.flatnonzero(perm == b)[0] for b in range(D0)])
    rep = first[perm]                                # the first copy of the base column that d holds
    big = [np.ascontiguousarray(x.reshape(N, D0)[:, perm].reshape(N, BIG_NLEV, BIG_NT)) for x in list(f) + [q]]
    plev_big = np.linspace(10.0, 1000.0, BIG_NLEV)
    tol = tol_of(L, dtype)
    label = "tiled cs8 x 26 x 50 L=%d %s" % (L, np.dtype(dtype).name)
    worst = [0.0]

    def column_wise(name, x, ref):
        """x [.][26][50] against column perm[d] of ref [.][7][3]; every copy of a base column bitwise the same."""
        x = x.reshape(x.shape[0], D)
        ref = ref.reshape(ref.shape[0], D0)[:, perm]
        e = err(x, ref)
        worst[0] = max(worst[0], e)
        assert e <= tol, (label, name, e, tol)
        assert np.array_equal(np.isnan(x), np.isnan(ref)), (label, name)
        assert np.array_equal(x, x[:, rep], equal_nan=True), (label, name, "copies of a base column differ")

    plan, dev, out = run_plan(lat, plev_big, big[:4], L)
    qd, tres, tzon, tcov = tracer_out(plan, dev, big[4])
    del tres
    assert not plan.status()
    column_wise("tracer coverage", tcov, to.coverage)
    for i, n in enumerate(TRACER_ZONAL[:3]):
        column_wise(n, tzon[i], to.zonal[n])
    column_wise("coverage", out["cov"], to.mo.coverage)
    for n in TEM_ZONAL_BY_COLUMN:
        column_wise(n, out["zon"][ZONAL.index(n)], to.mo.zonal[n])
    eddy = plan.tracer_eddy_masked(qd, dev[1], dev[3])
    for n in TRACER_NATIVE:
        column_wise(n, eddy.pop(n).cpu().numpy(), to.native[n])
    del eddy
    eddy = plan.tem_eddy(*dev, names=TEM_NATIVE_BY_COLUMN)
    for n in TEM_NATIVE_BY_COLUMN:
        column_wise(n, eddy.pop(n).cpu().numpy(), to.mo.native[n])
    print("%s: worst error %.2e (bound %.1e)" % (label, worst[0], tol))


# ---- 4. ranges shorter than the ring --------------------------------------------------------------------------------
@pytest.mark.parametrize("nlat,nlon,L,dtype", [(18, 2, 12, F64), (18, 2, 12, F32), (18, 2, 7, F64), (13, 1, 3, F64)])
def test_ranges_shorter_than_the_ring(nlat, nlon, L, dtype):
    lat, lon, plev, f, q, to = small_case(nlat, nlon, L, dtype)
    assert lat.size == nlat * nlon and f[0].shape[1:] == (3, 1)
    label = "cap latlon(%d, %d) x 3 x 1 L=%d %s" % (nlat, nlon, L, np.dtype(dtype).name)
    check_run(label, lat, plev, f, q, to, L, tight(dtype))


# ---- 5. two paths, one fit ------------------------------------------------------------------------------------------
SAME_FIT = [("scattered", L, dt) for L in (15, 31, 51, 63) for dt in (F64, F32)]
SAME_FIT += [("cap", L, dt) for L in (20, 50, 63) for dt in (F64, F32)]


@pytest.mark.parametrize("mask,L,dtype", SAME_FIT)
def test_tracer_path_equals_tem_path_on_the_same_fit(mask, L, dtype):
    lat, lon = grid("cs8")
    if mask == "scattered":
        plev, f, _ = scattered_fields(lat, lon, NLEV, NT, dtype=dtype)
        thr, tol = 0.0, 1e-11
    else:
        plev, f, _ = masked_tracer_fields(lat, lon, NLEV, NT, dtype=dtype, gap=False)
        thr, tol = THR, (1e-11 if L == 20 else tol_of(L, dtype))
    label = "same fit, %s cs8 L=%d %s" % (mask, L, np.dtype(dtype).name)
    plan, dev, out = run_plan(lat, plev, f, L, min_coverage=thr)
    qd, tres, tzon, tcov = tracer_out(plan, dev, f[0])         # the tracer is ua: its mask is the common mask
    worst = 0.0
    pairs = [("coverage", tcov, out["cov"])]
    pairs += [(n, tzon[i], out["zon"][ZONAL.index(m)]) for i, (n, m) in enumerate((("qb", "ub"), ("qpvpb", "upvpb"),
                                                                                  ("qpwappb", "upwappb")))]
    teddy = plan.tracer_eddy_masked(qd, dev[1], dev[3])
    eddy = plan.tem_eddy(*dev, names=("up", "upvp", "upwapp"))
    pairs += [(n, teddy[n].cpu().numpy(), eddy[m].cpu().numpy()) for n, m in (("qp", "up"), ("qpvp", "upvp"),
                                                                              ("qpwapp", "upwapp"))]
    for n, x, ref in pairs:
        e = err(x, ref)
        worst = max(worst, e)
        assert e <= tol, (label, n, e, tol)
        assert np.array_equal(np.isnan(x), np.isnan(ref)), (label, n)
    assert np.isfinite(tzon[0]).any() and (mask == "scattered" or np.isnan(tzon[0]).any())
    print("%s: worst difference %.2e (bound %.1e)" % (label, worst, tol))
