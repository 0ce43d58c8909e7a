"""Grouped and weighted time means on the MI355X: the grouped sum (temxg_time_sum_groups) and
``TEMDiagnostics(..., climatology=True, time_groups=g, time_weights=w)``.

Bounds.
  * grouped sum against numpy fp64, per (row, group): |got - ref| <= 2 (n_g + 1) 2^-53 sum_{t in g} |w_t x_t| with n_g the
    times of the group in the block.  A product w_t x_t rounds once (2^-53 relative, or not at all inside an fma), any
    order of n_g fp64 additions is within (n_g - 1) 2^-53 sum|w x| of the exact sum to first order, so kernel and
    reference are each within n_g 2^-53 sum|w x| and differ by at most twice that; the +1 covers the second-order
    terms.  Derived, not measured.  Bitwise where the contract says so (one time per group, repeated calls, equal rows).
  * front end against the numpy oracle: 1e-10 field-normalised for fp64 (the project's oracle bound), 2e-5 for fp32
    fields; two GPU routes that differ in summation order only: 1e-11; stationary + transient = total for the four
    flux-linear results: 1e-12.  Transient quantities and the four linear results of every set are normalised by the
    TOTAL's maximum, as ``compare`` of tests/test_gpu_clim.py does, because they are differences.
References: tests/test_gclim_host.py, gclim_reference (the oracle on the group-mean fields, and its epilogue on the group
means of the per-snapshot zonal means)."""
import ctypes as C

import numpy as np
import pytest

from test_gclim_host import LABELS, LINEAR, WEIGHTS, ZM7, gclim_reference
from test_gpu_clim import CANARY, as_dicts, grid, off_by_one, oracle_values, small_plan, tensors, values

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
SETS = ("total", "stationary", "transient")
SHAPES = ((1, 1), (37, 3), (866, 6))
NGS = (1, 5, 64)
_cache = {}


def switch(dtype):
    from pytemdiags_amd import _gclim
    return _gclim.switch_nt(np.dtype(dtype).itemsize)


def nts_of(dtype):
    s = switch(dtype)
    return sorted({1, 2, 3, 15, 16, 17, 31, 33, 63, 64, 65, 129, s - 1, s, s + 1, 1000})


def make_labels(kind, nt, ng, rng):
    if kind == "contiguous":                       # month-like: ng runs of about equal length
        return ((np.arange(nt) * ng) // nt).astype(np.int32)
    lab = rng.integers(0, ng, nt).astype(np.int32)
    lab[rng.random(nt) < 0.1] = -1
    return lab


def make_weights(nt, rng):
    w = rng.uniform(0.0, 2.0, nt)
    w[rng.random(nt) < 0.15] = 0.0
    return w


def reference(x, labels, ng, weights):
    """-> (sums, bounds), each ``x.shape[:-1] + (ng,)``, over the labelled times of ``x`` (all of it is one block)."""
    x64 = np.asarray(x, dtype=np.float64)
    nt = x64.shape[-1]
    w = np.ones(nt) if weights is None else np.asarray(weights, dtype=np.float64)
    ref = np.zeros(x64.shape[:-1] + (ng,))
    mag = np.zeros_like(ref)
    n = np.zeros(ng)
    for g in range(ng):
        idx = np.nonzero(labels == g)[0]
        n[g] = idx.size
        if idx.size:
            with np.errstate(invalid="ignore"):
                ref[..., g] = (x64[..., idx] * w[idx]).sum(-1)
                mag[..., g] = np.abs(x64[..., idx] * w[idx]).sum(-1)
    return ref, 2.0 * (n + 1.0) * 2.0 ** -53 * mag


class Guarded:
    """fp64 accumulators ``[ncol][nlev][ng]``, each a view one element into a buffer of its own full of canaries (or
    of ``prefill`` values between the canaries)."""

    def __init__(self, n, ncol, nlev, ng, prefill=None):
        m = ncol * nlev * ng
        self.bufs = [torch.full((m + 4,), CANARY, dtype=torch.float64, device=DEV) for _ in range(n)]
        self.acc = [b[1:1 + m].view(ncol, nlev, ng) for b in self.bufs]
        self.m = m
        if prefill is not None:
            for a in self.acc:
                a.copy_(torch.as_tensor(prefill, device=DEV))

    def check(self):
        for b in self.bufs:
            edge = torch.cat([b[:1], b[1 + self.m:]]).cpu().numpy()
            assert np.all(edge == CANARY), "a canary next to an accumulator was overwritten"

    def numpy(self):
        return [a.cpu().numpy().copy() for a in self.acc]


def gsum(fields, labels, ng, weights=None, t0=0, into=None, accumulate=False, prefill=None):
    """-> (sums as numpy, the Guarded accumulators); sources and accumulators unaligned, canaries checked."""
    plan = small_plan()
    ncol, nlev, _ = fields[0].shape
    g = into or Guarded(len(fields), ncol, nlev, ng, prefill)
    out = plan.time_sum_groups([off_by_one(x) for x in fields], labels, ng, weights, t0=t0, acc=g.acc, accumulate=accumulate)
    assert all(o is a for o, a in zip(out, g.acc))
    torch.cuda.synchronize()
    g.check()
    return g.numpy(), g


# ---- temxg_time_sum_groups ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "contiguous"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_grouped_sum_parity_every_shape_unaligned_with_canaries(dtype, kind):
    rng = np.random.default_rng(17)
    worst = 0.0
    rows = SHAPES[-1][0] * SHAPES[-1][1]
    for nt in nts_of(dtype):
        big = (rng.standard_normal((rows, nt)) * 10.0 ** rng.integers(-3, 4, (rows, 1))).astype(dtype)
        for ng in NGS:
            labels = make_labels(kind, nt, ng, rng)
            for weights in (None, make_weights(nt, rng)):
                ref, tol = reference(big, labels, ng, weights)
                small = {}
                for ncol, nlev in SHAPES:
                    x = big[:ncol * nlev].reshape(ncol, nlev, nt)
                    (got,), _ = gsum([x], labels, ng, weights)
                    assert got.shape == (ncol, nlev, ng) and got.dtype == np.float64
                    got = got.reshape(ncol * nlev, ng)
                    err = np.abs(got - ref[:ncol * nlev]) - tol[:ncol * nlev]
                    assert np.all(err <= 0), (nt, ng, ncol, nlev, weights is None, float(err.max()))
                    worst = max(worst, float(np.max(np.abs(got - ref[:ncol * nlev]) / np.maximum(tol[:ncol * nlev], 1e-300))))
                    absent = [g for g in range(ng) if not np.any(labels == g)]
                    assert np.all(got[:, absent] == 0) and not np.any(np.signbit(got[:, absent]))
                    if (ncol, nlev) == SHAPES[-1]:
                        (again,), _ = gsum([x], labels, ng, weights)          # repeated calls: identical bits
                        assert again.tobytes() == got.tobytes()
                        # equal rows give equal bits whatever ncol, nlev and the row's position
                        for m, s in small.items():
                            assert s.tobytes() == got[:m].tobytes(), (nt, ng, m)
                    else:
                        small[ncol * nlev] = got
    print("%s %s: worst |delta| / bound %.3f over nt in %s" % (np.dtype(dtype).name, kind, worst, nts_of(dtype)))


@pytest.mark.parametrize("nt", [1, 7, 64])
def test_one_time_per_group_is_a_bit_copy(nt):
    rng = np.random.default_rng(nt)
    special = np.array([-0.0, 0.0, 5e-324, -5e-324, np.finfo(np.float64).max, -np.finfo(np.float64).max,
                        np.float64(np.float32(1e-45)), 2.2250738585072014e-308])
    x = rng.standard_normal((37, 3, nt))
    x.reshape(-1)[:: 5] = special[rng.integers(0, special.size, x.reshape(-1)[:: 5].size)]
    perm = rng.permutation(nt).astype(np.int32)
    (got,), _ = gsum([x], perm, nt)
    want = np.empty_like(x)
    want[..., perm] = x
    assert got.tobytes() == want.tobytes()
    s32 = np.array([-0.0, 0.0, 1e-45, -1e-45, np.finfo(np.float32).max, 3.25], dtype=np.float32)
    x32 = rng.standard_normal((37, 3, nt)).astype(np.float32)
    x32.reshape(-1)[:: 4] = s32[rng.integers(0, s32.size, x32.reshape(-1)[:: 4].size)]
    (got,), _ = gsum([x32], perm, nt)
    want = np.empty((37, 3, nt))
    want[..., perm] = x32.astype(np.float64)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_no_weights_is_an_array_of_ones_and_halved_weights_halve_the_sums(dtype):
    for nt in (17, 129, switch(dtype) + 1):
        rng = np.random.default_rng(nt)
        x = rng.standard_normal((37, 3, nt)).astype(dtype)
        labels = make_labels("random", nt, 5, rng)
        (plain,), _ = gsum([x], labels, 5)
        (ones,), _ = gsum([x], labels, 5, np.ones(nt))
        (half,), _ = gsum([x], labels, 5, np.full(nt, 0.5))
        assert plain.tobytes() == ones.tobytes(), nt
        assert half.tobytes() == (0.5 * plain).tobytes(), nt           # powers of two are exact


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_absent_groups_are_zero_or_keep_their_bits_under_accumulate(dtype):
    from pytemdiags_amd import _gclim
    for nt in (30, switch(dtype) + 3):
        rng = np.random.default_rng(nt)
        ncol, nlev, ng = 37, 3, 12
        x = rng.standard_normal((ncol, nlev, nt)).astype(dtype)
        labels = np.where(np.arange(nt) < nt // 2, 3, 7).astype(np.int32)       # two of the twelve groups
        labels[1] = -1
        pre = rng.standard_normal((ncol, nlev, ng)) * 1e3
        (fresh,), _ = gsum([x], labels, ng)
        absent = [g for g in range(ng) if g not in (3, 7)]
        assert np.all(fresh[..., absent] == 0) and np.all(fresh[..., [3, 7]] != 0)
        (acc,), _ = gsum([x], labels, ng, accumulate=True, prefill=pre)
        assert acc[..., absent].tobytes() == pre[..., absent].tobytes()              # neither read nor written
        assert acc[..., [3, 7]].tobytes() == (pre[..., [3, 7]] + fresh[..., [3, 7]]).tobytes()   # one further rounding
        # a block whose labels are all -1
        none = np.full(nt, -1, dtype=np.int32)
        (z,), _ = gsum([x], none, ng)
        assert np.all(z == 0) and not np.any(np.signbit(z))
        (kept,), _ = gsum([x], none, ng, accumulate=True, prefill=pre)
        assert kept.tobytes() == pre.tobytes()
        assert _gclim.bound(2) == 4


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_non_finite_values_poison_their_own_row_and_group_only(dtype):
    for nt in (17, switch(dtype) + 1):
        rng = np.random.default_rng(5)
        x = rng.standard_normal((37, 3, nt)).astype(dtype)
        labels = (np.arange(nt) % 3).astype(np.int32)
        labels[4] = -1
        w = np.ones(nt)
        w[6] = 0.0                                          # labels[6] == 0
        (clean,), _ = gsum([x], labels, 3, w)
        y = x.copy()
        y[5, 1, 7] = np.nan                                 # group 1
        y[20, 2, 0] = np.inf                                # group 0
        y[36, 2, nt - 1] = -np.inf                          # group (nt - 1) % 3
        y[9, 0, 4] = np.nan                                 # left out: poisons nothing
        y[11, 1, 6] = np.nan                                # weight 0 still multiplies: poisons group 0 of its row
        (got,), _ = gsum([y], labels, 3, w)
        hit = np.zeros((37, 3, 3), dtype=bool)
        hit[5, 1, 1] = hit[20, 2, 0] = hit[36, 2, (nt - 1) % 3] = hit[11, 1, 0] = True
        assert np.isnan(got[5, 1, 1]) and got[20, 2, 0] == np.inf and got[36, 2, (nt - 1) % 3] == -np.inf
        assert np.isnan(got[11, 1, 0])
        assert np.all(np.isfinite(got[~hit])) and got[~hit].tobytes() == clean[~hit].tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_permuting_rows_permutes_the_bits(dtype):
    for nt in (30, 129, switch(dtype), 1000):
        rng = np.random.default_rng(nt)
        x = rng.standard_normal((111, nt)).astype(dtype)
        labels, w = make_labels("random", nt, 5, rng), make_weights(nt, rng)
        perm = rng.permutation(111)
        (a,), _ = gsum([x.reshape(37, 3, nt)], labels, 5, w)
        (b,), _ = gsum([x[perm].reshape(37, 3, nt)], labels, 5, w)
        (c,), _ = gsum([x[perm].reshape(111, 1, nt)], labels, 5, w)
        (d,), _ = gsum([x[perm].reshape(1, 111, nt)], labels, 5, w)
        assert a.reshape(111, 5)[perm].tobytes() == b.tobytes() == c.tobytes() == d.tobytes(), nt


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_form_of_the_long_row_kernel_changes_no_bit(dtype):
    """The groups present in a block pick the long-row kernel (registers for at most 1 and at most 4, accumulators in
    LDS beyond); a (row, group) sum is the same bits in each: a group keeps its times while more and more of the other
    times, left out at first, are given to further groups."""
    from pytemdiags_amd import _gclim
    nt = switch(dtype) + 41
    rng = np.random.default_rng(8)
    x = rng.standard_normal((37, 3, nt)).astype(dtype)
    w = make_weights(nt, rng)
    base = rng.integers(0, 8, nt).astype(np.int32)
    got = {}
    for present in (1, 2, 4, 8):                      # the groups below `present` keep their times, the others are left out
        labels = np.where(base < present, base, -1).astype(np.int32)
        assert np.unique(labels[labels >= 0]).size == present
        (got[present],), _ = gsum([x], labels, 8, w)
    assert sorted(got) == [1, 2, 4, 8] and [_gclim.bound(n) for n in sorted(got)] == [1, 4, 4, 64]
    assert got[1][..., 0].tobytes() == got[2][..., 0].tobytes() == got[4][..., 0].tobytes() == got[8][..., 0].tobytes()
    assert got[2][..., 1].tobytes() == got[4][..., 1].tobytes() == got[8][..., 1].tobytes()
    assert got[4][..., 2:4].tobytes() == got[8][..., 2:4].tobytes()
    ref, tol = reference(x, base, 8, w)
    assert np.all(np.abs(got[8] - ref) <= tol)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_blocks_with_t0_accumulate_within_the_bound_of_the_whole_record(dtype):
    for nt in (50, switch(dtype) + 7):
        rng = np.random.default_rng(nt)
        x = rng.standard_normal((37, 6, nt)).astype(dtype)
        labels, w = make_labels("contiguous", nt, 4, rng), make_weights(nt, rng)     # the groups cross the cuts
        labels[3] = -1
        ref, tol = reference(x, labels, 4, w)
        (whole,), _ = gsum([x], labels, 4, w)
        g = None
        for t0, t1 in ((0, 13), (13, 14), (14, nt)):
            blk = np.ascontiguousarray(x[..., t0:t1])
            (now,), g = gsum([blk], labels, 4, w, t0=t0, into=g, accumulate=g is not None)
        assert np.all(np.abs(now - ref) <= tol) and np.all(np.abs(whole - ref) <= tol), nt
        (one,), _ = gsum([x], labels, 4, w, t0=0)
        assert one.tobytes() == whole.tobytes()
        # a block in the middle of the record, on its own: the sums of its own times only
        (mid,), _ = gsum([np.ascontiguousarray(x[..., 13:40])], labels, 4, w, t0=13)
        lab_mid = np.full(nt, -1, dtype=np.int32)
        lab_mid[13:40] = labels[13:40]
        mref, mtol = reference(x, lab_mid, 4, w)
        assert np.all(np.abs(mid - mref) <= mtol), nt


@pytest.mark.parametrize("nt", [17, 300])
def test_eight_fields_of_mixed_dtypes_in_one_call(nt):
    """nt = 300 lies between the two switch points: the fp64 fields take the long rows, the fp32 fields are staged."""
    assert switch(np.float64) <= 300 < switch(np.float32)
    rng = np.random.default_rng(nt)
    fields = [rng.standard_normal((37, 3, nt)).astype(np.float32 if f % 2 else np.float64) for f in range(8)]
    labels, w = make_labels("random", nt, 5, rng), make_weights(nt, rng)
    got, _ = gsum(fields, labels, 5, w)
    for f, (x, g) in enumerate(zip(fields, got)):
        ref, tol = reference(x, labels, 5, w)
        assert np.all(np.abs(g - ref) <= tol), f
        (alone,), _ = gsum([x], labels, 5, w)              # a sum does not depend on what else the call carries
        assert alone.tobytes() == g.tobytes(), f


def test_overlap_and_misalignment_are_refused_on_the_device():
    from pytemdiags_amd import _gclim
    lib = _gclim.load()
    ncol, nlev, nt, ng = 4, 3, 5, 2
    src = torch.zeros(ncol * nlev * nt + 32, dtype=torch.float64, device=DEV)      # room for 24 sums behind the source
    acc = torch.full((64,), CANARY, dtype=torch.float64, device=DEV)
    lab = (C.c_int32 * nt)(0, 1, -1, 1, 0)

    def call(s, a, dt=0, flags=0, nf=1, g=ng):
        sp = (C.c_void_p * nf)(*([s] if nf == 1 else s))
        ap = (C.c_void_p * nf)(*([a] if nf == 1 else a))
        return lib.temxg_time_sum_groups(0, nf, sp, (C.c_int * nf)(*([dt] * nf)), ap, ncol, nlev, nt, nt, 0, g, lab, None,
                                         flags, None)
    assert call(src.data_ptr(), src.data_ptr() + 8 * (ncol * nlev * nt - 1)) == -1 and b"overlaps src" in lib.temx_last_error()
    assert call(src.data_ptr(), src.data_ptr()) == -1
    assert call(src.data_ptr() + 8 * 24, src.data_ptr() + 8) == -1          # 24 doubles of acc reach into the src
    assert call([src.data_ptr(), src.data_ptr()], [acc.data_ptr(), acc.data_ptr() + 8 * 23], nf=2) == -1
    assert b"overlaps acc" in lib.temx_last_error()
    assert call(src.data_ptr() + 4, acc.data_ptr()) == -1 and b"aligned" in lib.temx_last_error()
    assert call(src.data_ptr(), acc.data_ptr() + 4) == -1 and b"aligned" in lib.temx_last_error()
    assert call(src.data_ptr() + 2, acc.data_ptr(), dt=1) == -1
    assert call(src.data_ptr(), acc.data_ptr(), flags=4) == -1
    assert call(src.data_ptr(), acc.data_ptr(), g=1) == -1 and b"label" in lib.temx_last_error()
    torch.cuda.synchronize()
    assert torch.all(acc == CANARY)                                        # a refused call wrote nothing
    assert call(src.data_ptr() + 4, acc.data_ptr() + 8, dt=1) == 0           # fp32 at 4 mod 8
    assert call(src.data_ptr(), src.data_ptr() + 8 * ncol * nlev * nt) == 0  # touching, not overlapping
    torch.cuda.synchronize()
    assert torch.all(acc[1:25] == 0) and acc[0] == CANARY and torch.all(acc[25:] == CANARY)
    assert torch.all(src == 0)


# ---- front end ----------------------------------------------------------------------------------------------------------
def front_case(kind, dtype=np.float64, L=20, nlev=6, labels=LABELS, weights=WEIGHTS, tag="std"):
    """(lat, plev, fields, reference) of one front-end case at nt = 7: computed once, shared, left unchanged."""
    key = ("front", kind, np.dtype(dtype).name, L, nlev, tag)
    if key not in _cache:
        from pytemdiags_amd import synth
        lat, lon = grid(kind)
        plev = synth.pressure_levels(nlev)
        f = [x.astype(dtype) for x in synth.analytic_fields(lat, lon, plev, 7, seed=5)]
        for x in f:
            x.setflags(write=False)
        _cache[key] = (lat, plev, f, gclim_reference(f, lat, plev, L, labels, weights))
    return _cache[key]


def compare(got, want, total, tol, tag, G):
    """``got``, ``want``: {set: {name: array (lat, plev, G)}}; ``total``: the reference's total set, whose maxima normalise
    the transient set and the four linear results of every set."""
    worst = (0.0, "")
    for s in SETS:
        for n, r in want[s].items():
            x = got[s][n]
            assert x.shape == r.shape == (r.shape[0], r.shape[1], G), (s, n, x.shape, r.shape)
            den = np.max(np.abs(total[n] if (s == "transient" or n in LINEAR) else r))
            e = float(np.max(np.abs(x - r)) / den)
            worst = max(worst, (e, "%s.%s" % (s, n)))
            assert e <= tol, (tag, s, n, e)
    print("%s: worst normalised error %.2e (%s)" % (tag, worst[0], worst[1]))
    return worst[0]


def wanted(ref):
    return {"total": oracle_values(ref["sets"]["total"]), "stationary": oracle_values(ref["stat"]),
            "transient": oracle_values(ref["sets"]["transient"])}


def check_against_oracle(cl, ref, tol, tag, G):
    want = wanted(ref)
    got = {s: values(getattr(cl, s)) for s in SETS}
    compare(got, want, want["total"], tol, tag, G)
    for n in LINEAR:           # stationary + transient = total for the results linear and homogeneous in the fluxes
        e = float(np.max(np.abs(got["stationary"][n] + got["transient"][n] - got["total"][n])) / np.max(np.abs(got["total"][n])))
        assert e <= 1e-12, (tag, n, e)
    for n in ZM7[:4]:          # the sets share the mean state
        assert np.array_equal(got["total"][n], got["stationary"][n]) and np.array_equal(got["total"][n], got["transient"][n])
    return got


def build(kind, dtype=np.float64, L=20, fields=None, **kw):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f, ref = front_case(kind, dtype, L)
    return TEMDiagnostics(*(f if fields is None else fields), lat, plev=plev, L=L, debug_level=0, **kw), ref


GROUPED = dict(climatology=True, time_groups=LABELS, time_weights=WEIGHTS)


@pytest.mark.parametrize("kind,kw", [("cs8", {}), ("random", {}), ("random", {"lat_bins": True}), ("cs4", {"L": 30})],
                         ids=["cs8-classes", "random-generic", "random-binned", "cs4-L30"])
def test_grouped_climatology_matches_the_oracle(kind, kw):
    from pytemdiags_amd import climatology
    tem, ref = build(kind, **GROUPED, **kw)
    cl = tem.climatology
    assert isinstance(cl, climatology.TEMClimatology) and cl.nt == 7
    if kind == "random":
        assert tem.sweep_form == ("binned" if kw.get("lat_bins") else "two-pass")
    check_against_oracle(cl, ref, 1e-10, "%s %s" % (kind, kw), 2)
    np.testing.assert_array_equal(cl.groups, [0, 1])
    assert cl.group_names == [0, 1]
    np.testing.assert_array_equal(cl.group_counts, [2, 4])
    np.testing.assert_array_equal(cl.group_weights, [0.75, 4.0])
    np.testing.assert_allclose(cl.time, [(0.5 * 1 + 0.25 * 4) / 0.75, (2 * 3 + 5) / 4.0], rtol=1e-15)
    assert cl.time_sum_path == ("kernel" if climatology.GROUP_SUM_KERNEL["float64"] else "torch")
    assert cl.total.epfy().shape == (180, 6, 2)


def test_grouped_climatology_of_fp32_fields():
    from pytemdiags_amd import climatology
    tem, ref = build("cs4", np.float32, **GROUPED)
    cl = tem.climatology
    assert cl.total.epfy().dtype == np.float32 and cl.total.psi.dtype == np.float64 and cl.transient.vtem().dtype == np.float32
    assert cl.time_sum_path == ("kernel" if climatology.GROUP_SUM_KERNEL["float32"] else "torch")
    want = wanted(ref)
    compare({s: values(getattr(cl, s)) for s in SETS}, want, want["total"], 2e-5, "cs4 fp32", 2)


def test_a_group_equals_the_plain_climatology_of_its_times():
    lat, plev, f, _ = front_case("cs4")
    labels = np.array([1, 0, -1, 1, 0, 1, 1])
    grouped, _ = build("cs4", climatology=True, time_groups=labels)
    G = as_dicts(tensors(grouped.climatology))
    for g in range(2):
        sub = [np.ascontiguousarray(x[..., labels == g]) for x in f]
        alone, _ = build("cs4", fields=sub, climatology=True)
        A = as_dicts(tensors(alone.climatology))
        mine = {s: {n: v[..., g:g + 1] for n, v in G[s].items()} for s in SETS}
        compare(mine, A, A["total"], 1e-11, "group %d against its own climatology" % g, 1)
    zeros, _ = build("cs4", climatology=True, time_groups=np.zeros(7, dtype=int))
    plain, _ = build("cs4", climatology=True)
    P = as_dicts(tensors(plain.climatology))
    compare(as_dicts(tensors(zeros.climatology)), P, P["total"], 1e-11, "one group of everything against climatology=True", 1)
    np.testing.assert_array_equal(zeros.climatology.time, plain.climatology.time)


def test_weights_alone_give_one_weighted_group():
    lat, plev, f, _ = front_case("cs4")
    w = np.array([31, 28, 31, 30, 31, 30, 31.0])
    key = ("ref", "cs4-weights")
    if key not in _cache:
        _cache[key] = gclim_reference(f, lat, plev, 20, np.zeros(7, dtype=int), w)
    tem, _ = build("cs4", climatology=True, time_weights=w)
    cl = tem.climatology
    assert cl.total.vtem().shape == (180, 6, 1) and cl.group_names == [0] and cl.group_weights[0] == 212
    check_against_oracle(cl, _cache[key], 1e-10, "weights alone", 1)


def test_labelled_input_with_dates_grouped_by_month():
    from pytemdiags_amd import LabeledArray, TEMDiagnostics
    lat, plev, f, _ = front_case("cs4")
    t = np.array(["2001-12-30", "2001-12-31", "2002-01-01", "2002-01-03", "2002-02-01", "2002-12-05", "2003-01-09"],
                 dtype="datetime64[D]")
    lab = [LabeledArray(x, ("ncol", "plev", "time"), {"plev": plev, "time": t}, name=n)
           for x, n in zip(f, ("ua", "va", "ta", "wap"))]
    tem = TEMDiagnostics(*lab, lat, L=20, debug_level=0, climatology=True, time_groups="month")
    cl = tem.climatology
    assert cl.group_names == ["Jan", "Feb", "Dec"]
    np.testing.assert_array_equal(cl.group_counts, [3, 1, 3])
    # the mean dates: Jan {2002-01-01, 2002-01-03, 2003-01-09} -> 2002-01-01 + (0 + 2 + 373) / 3 days
    assert list(cl.time) == [np.datetime64("2002-05-06"), np.datetime64("2002-02-01"),
                             np.datetime64("2001-12-30") + np.timedelta64(int(np.rint((0 + 1 + 340) / 3)), "D")]
    x = cl.transient.epdiv()
    assert x.dims == ("lat", "plev", "time") and x.values.shape == (180, 6, 3)
    assert cl.stationary.ub.dims == ("lat", "plev", "time")
    raw, _ = build("cs4", climatology=True, time_groups=np.array([2, 2, 0, 0, 1, 2, 0]))
    for s, (res, zon) in tensors(raw.climatology).items():
        assert res.tobytes() == tensors(cl)[s][0].tobytes() and zon.tobytes() == tensors(cl)[s][1].tobytes(), s
    season = TEMDiagnostics(*lab, lat, L=20, debug_level=0, climatology=True, time_groups="season").climatology
    assert season.group_names == ["DJF"] and season.total.epfy().values.shape == (180, 6, 1)


@pytest.mark.parametrize("source", ["device", "host-time-major"])
def test_blocked_grouped_climatology_against_the_whole_run(source):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f, ref = front_case("cs4")
    whole, _ = build("cs4", **GROUPED)
    want = as_dicts(tensors(whole.climatology))
    if source == "device":
        args, kw = [torch.as_tensor(x, device=DEV) for x in f], {}
    else:
        args, kw = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in f], {"dims": ("time", "plev", "ncol")}
    kw.update(plev=plev, L=20, debug_level=0, **GROUPED)
    two = TEMDiagnostics(*args, lat, time_block=2, **kw)          # blocks [0,2) [2,4) [4,6) [6,7): both groups cross them
    assert two.climatology.nt == 7 and two.climatology.time_sum_path == whole.climatology.time_sum_path
    compare(as_dicts(tensors(two.climatology)), want, want["total"], 1e-11, "time_block=2 from %s" % source, 2)
    check_against_oracle(two.climatology, ref, 1e-10, "time_block=2 from %s, oracle" % source, 2)
    with pytest.raises(RuntimeError, match="time_block"):
        two.up
    seven = TEMDiagnostics(*args, lat, time_block=7, **kw)
    for s, (res, zon) in tensors(seven.climatology).items():
        assert res.tobytes() == tensors(whole.climatology)[s][0].tobytes(), s
        assert zon.tobytes() == tensors(whole.climatology)[s][1].tobytes(), s


@pytest.mark.parametrize("kind", ["cs8", "random"])
def test_per_snapshot_run_and_native_outputs_are_those_of_an_object_without_the_keywords(kind):
    from pytemdiags_amd import TEMDiagnostics, _lib, synth
    lat, plev, f, _ = front_case(kind)
    lon = grid(kind)[1]
    q = synth.analytic_tracer(lat, lon, plev, 7, which=0)
    plain = TEMDiagnostics(*f, lat, plev=plev, L=20, debug_level=0, q=q)
    tem = TEMDiagnostics(*f, lat, plev=plev, L=20, debug_level=0, q=q, **GROUPED)
    assert tem.climatology.nt == 7 and tem.climatology.total.epfy().shape == (180, 6, 2)
    assert torch.equal(tem._res, plain._res) and torch.equal(tem._zon, plain._zon)
    for n in _lib.RESULT_NAMES:
        np.testing.assert_array_equal(getattr(tem, n)(), getattr(plain, n)())
    for n in _lib.ZONAL_NAMES:
        np.testing.assert_array_equal(getattr(tem, n), getattr(plain, n))
    np.testing.assert_array_equal(tem.etfy(), plain.etfy())        # a tracer's results
    np.testing.assert_array_equal(tem.etdiv(), plain.etdiv())
    for n in ("up", "vp", "thetap", "wapp", "upvp", "upwapp", "vptp"):    # the plan's state is that of the ordinary run
        np.testing.assert_array_equal(getattr(tem, n), getattr(plain, n))
    np.testing.assert_array_equal(tem.qp[0], plain.qp[0])
    np.testing.assert_array_equal(tem.qpvp[0], plain.qpvp[0])


def test_from_model_levels_passes_the_group_keywords_through():
    from test_vertical_host import PLEV37, frontend_case, hybrid_pressure, inside_everywhere
    from pytemdiags_amd import TEMDiagnostics, interp_to_pressure
    lat, lon, hyam, hybm, ps, f = frontend_case()
    nt = f[0].shape[2]
    levels = PLEV37[inside_everywhere(hybrid_pressure(hyam, hybm, ps), PLEV37 * 100.0)]
    labels, w = np.arange(nt) % 2, np.linspace(0.5, 2.0, nt)
    kw = dict(L=30, debug_level=0, climatology=True, time_groups=labels, time_weights=w)
    a = TEMDiagnostics.from_model_levels(*f, lat, plev=levels, ps=ps, hyam=hyam, hybm=hybm, **kw)
    g = interp_to_pressure(f, levels, ps=ps, hyam=hyam, hybm=hybm)
    b = TEMDiagnostics(*g, lat, plev=levels, **kw)
    G = int(labels.max()) + 1
    assert a.climatology.nt == b.climatology.nt == nt and a.climatology.total.epfy().shape[2] == G
    ta, tb = tensors(a.climatology), tensors(b.climatology)
    for s in SETS:
        assert ta[s][0].tobytes() == tb[s][0].tobytes() and ta[s][1].tobytes() == tb[s][1].tobytes(), s
    np.testing.assert_array_equal(a.up, b.up)
    # time-major model levels, fed by a block source
    tm = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in f]
    c = TEMDiagnostics.from_model_levels(*tm, lat, plev=levels, ps=np.ascontiguousarray(ps.T), hyam=hyam, hybm=hybm,
                                         dims=("time", "lev", "ncol"), **kw)
    assert c.climatology.nt == nt
    want = as_dicts(tb)
    compare(as_dicts(tensors(c.climatology)), want, want["total"], 1e-10, "time-major model levels", G)


@pytest.mark.parametrize("kind", ["random", "cs4"])
def test_group_sum_path_follows_the_gate_and_the_two_paths_agree(kind, monkeypatch):
    """The two paths differ in the order of their fp64 operations only (fma chains in ascending time against a matrix
    product); 1e-11 is the project's bound between two such routes."""
    from pytemdiags_amd import climatology
    runs = {}
    for on in (True, False):
        monkeypatch.setattr(climatology, "GROUP_SUM_KERNEL", {"float64": on, "float32": on})
        t, _ = build(kind, **GROUPED)
        assert t.climatology.time_sum_path == ("kernel" if on else "torch")
        runs[on] = as_dicts(tensors(t.climatology))
    compare(runs[True], runs[False], runs[False]["total"], 1e-11, "kernel path against torch path, %s" % kind, 2)
