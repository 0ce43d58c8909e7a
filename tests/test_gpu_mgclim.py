"""Masked grouped time means on the MI355X: the grouped, weighted sum over the valid times
(temxw_time_sum_groups_valid, ``Plan.time_sum_groups_valid``).

Bounds.
  * bit pinning against the grouped sum that exists without this feature (temxg_time_sum_groups): ``acc`` equals by
    value its sums of the source with every invalid element (under the applicable mask) replaced by +0.0, ``wsum`` its
    sums of the indicator field, ``cnt`` those with weights None; ``np.array_equal``, so only the sign of a zero may
    differ.  The indicator has the dtype of the call: the order of the parent's additions is a function of (nt, dtype)
    -- staged below 256 times for fp64 and below 512 for fp32 -- so an fp64 indicator of an fp32 call with
    256 <= nt < 512 goes through the parent's other form and pins another order than the one ``acc`` is pinned to.
    Where the two forms coincide the fp64 indicator is compared as well.
  * against numpy fp64, per (row, group): |got - ref| <= 2 (n_g + 1) 2^-53 sum |w_t x_t| over the valid times of the
    group (``test_gpu_gclim.reference``: derived there, not measured); ``cnt`` exact.
  * bitwise where the contract says so: one valid time of weight 1, repeated calls, permuted rows, the form of the
    kernel, absent groups under the flag.
Rows are tiny (37 x 3, two workgroups or more in every form); the nt values bracket the switch to the long-row forms
and the nt at which fewer than 16 rows of the workgroup's fields fit the staged images."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_clim import CANARY, off_by_one, small_plan
from test_gpu_gclim import Guarded, gsum, make_labels, make_weights, reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
NCOL, NLEV = 37, 3
MODES = ((1, False), (4, True), (8, True), (3, False))          # (nf, common mask)
NGS = (1, 3, 5, 24, 64)


def switch(dtype):
    from pytemdiags_amd import _mgclim
    return _mgclim.switch_nt(np.dtype(dtype).itemsize)


def nts_of(dtype, nf, common):
    from pytemdiags_amd import _nclim
    s = switch(dtype)
    few = _nclim.switch_nt(np.dtype(dtype).itemsize, nf, common)      # fewer than 16 rows fit from here on
    return sorted({1, 2, 5, 30, few - 1, few, s - 1, s, s + 1, 257, 300})


def holes(nf, nt, dtype, rng, labels=None):
    """nf fields ``[NCOL][NLEV][nt]`` with holes of their own: NaN and +-Inf at random, a NaN in one field only, a whole
    row missing, and a whole (row, group) missing."""
    out = []
    for f in range(nf):
        x = (rng.standard_normal((NCOL, NLEV, nt)) * 10.0 ** rng.integers(-3, 4, (NCOL, NLEV, 1))).astype(dtype)
        bad = rng.random(x.shape) < 0.08
        x[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf]), int(bad.sum())).astype(dtype)
        out.append(x)
    out[0][3, 1, :] = np.nan                                          # a whole row
    out[-1][7, 2, nt // 2] = np.nan                                   # one field only
    if labels is not None and np.any(labels >= 0):
        g = labels[labels >= 0][0]
        out[0][11, 0, labels == g] = np.inf                           # a whole (row, group)
    return out


def masks(fields, common):
    ok = [np.isfinite(x) for x in fields]
    if common:
        ok = [np.logical_and.reduce(ok)] * len(fields)
    return ok


def mgsum(fields, labels, ng, weights=None, t0=0, common=True, accumulate=False, prefill=None, into=None):
    """-> (acc, wsum, cnt as lists of numpy arrays, the three Guarded sets); sources and outputs unaligned, canaries
    around all three outputs checked."""
    plan = small_plan()
    ncol, nlev, _ = fields[0].shape
    n, nx = len(fields), (1 if common else len(fields))
    ga, gw, gc = into or (Guarded(n, ncol, nlev, ng, prefill), Guarded(nx, ncol, nlev, ng, prefill),
                          Guarded(nx, ncol, nlev, ng, prefill))
    acc, wsum, cnt = plan.time_sum_groups_valid([off_by_one(x) for x in fields], labels, ng, weights, t0=t0, acc=ga.acc,
                                                wsum=gw.acc if not common else gw.acc[0],
                                                cnt=gc.acc if not common else gc.acc[0], accumulate=accumulate,
                                                common=common)
    assert all(o is a for o, a in zip(acc, ga.acc))
    assert (wsum is gw.acc[0] and cnt is gc.acc[0]) if common else (len(wsum) == len(cnt) == n)
    torch.cuda.synchronize()
    for g in (ga, gw, gc):
        g.check()
    return ga.numpy(), gw.numpy(), gc.numpy(), (ga, gw, gc)


def pinned(fields, labels, ng, weights, common, t0=0, ind_dtype=None):
    """What the parent kernel gives on the derived inputs: (acc, wsum, cnt) as lists of numpy arrays."""
    ok = masks(fields, common)
    dt = fields[0].dtype
    zero = [np.where(m, x, dt.type(0)) for x, m in zip(fields, ok)]
    ind = [m.astype(ind_dtype or dt) for m in (ok[:1] if common else ok)]
    acc, _ = gsum(zero, labels, ng, weights, t0=t0)
    wsum, _ = gsum(ind, labels, ng, weights, t0=t0)
    cnt, _ = gsum(ind, labels, ng, None, t0=t0)
    return acc, wsum, cnt


# ---- bit pinning against the parent kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("nf,common", MODES, ids=["1own", "4common", "8common", "3own"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bits_are_those_of_the_grouped_sum_on_the_derived_inputs(dtype, nf, common):
    from pytemdiags_amd import _gclim, _mgclim
    rng = np.random.default_rng(23)
    forms = set()
    for nt in nts_of(dtype, nf, common):
        for i, ng in enumerate(NGS):
            for kind in ("random", "contiguous"):
                labels = make_labels(kind, nt, ng, rng)
                if nt > 2:
                    labels[rng.integers(0, nt)] = -1                              # a left-out time
                weights = make_weights(nt, rng)
                weights[rng.integers(0, nt)] = 0.0
                x = holes(nf, nt, dtype, rng, labels)
                acc, wsum, cnt, _ = mgsum(x, labels, ng, weights, common=common)
                pa, pw, pc = pinned(x, labels, ng, weights, common)
                where = (np.dtype(dtype).name, nf, common, nt, ng, kind)
                for f in range(nf):
                    assert np.array_equal(acc[f], pa[f]), ("acc", f) + where
                for f in range(len(wsum)):
                    assert np.array_equal(wsum[f], pw[f]), ("wsum", f) + where
                    assert np.array_equal(cnt[f], pc[f]), ("cnt", f) + where
                if (nt < _gclim.switch_nt(8)) == (nt < switch(dtype)) and dtype is np.float32 and kind == "random":
                    _, pw64, pc64 = pinned(x, labels, ng, weights, common, ind_dtype=np.float64)   # the fp64 indicator
                    for f in range(len(wsum)):
                        assert np.array_equal(wsum[f], pw64[f]) and np.array_equal(cnt[f], pc64[f]), ("ind64", f) + where
                npres = np.unique(labels[labels >= 0]).size
                sh = _mgclim.shape(NCOL * NLEV, nt, np.dtype(dtype).itemsize, _mgclim.staged_fields(nf, common), max(npres, 1))
                forms.add(("staged", sh["rpb"] >= 16) if sh["staged"] else (sh["bound"], sh["npass"] > 1))
    # every form ran: staged with many and with few rows, registers for 1 and 4, LDS, and (8 fields, 64 groups) batched
    want = {("staged", True), (1, False), (4, False), (64, False)}
    if _mgclim.staged_fields(nf, common) > 1:
        want.add(("staged", False))
    if nf == 8:
        want.add((64, True))
    assert want <= forms, (want - forms)


@pytest.mark.parametrize("nf,common", MODES, ids=["1own", "4common", "8common", "3own"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sums_weights_and_counts_against_numpy(dtype, nf, common):
    rng = np.random.default_rng(29)
    worst = 0.0
    for nt in (5, 30, switch(dtype) - 1, switch(dtype) + 1, 1000):
        for ng in (3, 24):
            labels, weights = make_labels("random", nt, ng, rng), make_weights(nt, rng)
            x = holes(nf, nt, dtype, rng, labels)
            acc, wsum, cnt, _ = mgsum(x, labels, ng, weights, common=common)
            ok = masks(x, common)
            for f in range(nf):
                ref, tol = reference(np.where(ok[f], x[f], 0).astype(np.float64), labels, ng, weights)
                assert np.all(np.abs(acc[f] - ref) <= tol), ("acc", f, nt, ng, float(np.max(np.abs(acc[f] - ref) - tol)))
                worst = max(worst, float(np.max(np.abs(acc[f] - ref) / np.maximum(tol, 1e-300))))
            for f in range(len(wsum)):
                ref, tol = reference(ok[f].astype(np.float64), labels, ng, weights)
                assert np.all(np.abs(wsum[f] - ref) <= tol), ("wsum", f, nt, ng)
                want = np.stack([ok[f][..., labels == g].sum(-1) for g in range(ng)], -1)
                assert np.array_equal(cnt[f], want.astype(np.float64)), ("cnt", f, nt, ng)       # exact
                assert np.all(np.isfinite(wsum[f])) and np.all(np.isfinite(acc[f]))
    print("%s nf=%d common=%s: worst |delta| / bound %.3f" % (np.dtype(dtype).name, nf, common, worst))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_valid_time_of_weight_one_is_a_bit_copy(dtype):
    if dtype is np.float64:
        special = np.array([-0.0, 0.0, 5e-324, -5e-324, np.finfo(np.float64).max, -np.finfo(np.float64).max,
                            2.2250738585072014e-308, 1.0])
    else:
        special = np.array([-0.0, 0.0, 1e-45, -1e-45, np.finfo(np.float32).max, -np.finfo(np.float32).max, 3.25, 1e-38],
                           dtype=np.float32)
    for nt in (7, 64, switch(dtype) + 5):
        rng = np.random.default_rng(nt)
        ng = min(nt // 2, 64)
        # group g holds the times g and g + ng; one of the two is missing in every row, which one varies
        labels = np.full(nt, -1, dtype=np.int32)
        labels[:2 * ng] = np.tile(np.arange(ng), 2)
        x = special[rng.integers(0, special.size, (NCOL, NLEV, nt))].astype(dtype)
        keep = rng.integers(0, 2, (NCOL, NLEV, ng))
        want = np.where(keep == 0, x[..., :ng], x[..., ng:2 * ng]).astype(np.float64)
        y = x.copy()
        y[..., :ng][keep == 1] = np.nan
        y[..., ng:2 * ng][keep == 0] = -np.inf
        for common in (True, False):
            (acc,), (wsum,), (cnt,), _ = mgsum([y], labels, ng, None, common=common)
            assert acc.tobytes() == want.tobytes(), (nt, common)
            assert np.all(wsum == 1.0) and np.all(cnt == 1.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_invalid_times_of_weight_zero_and_left_out_times_touch_nothing(dtype):
    for nt in (17, switch(dtype) + 1):
        rng = np.random.default_rng(5)
        x = [rng.standard_normal((NCOL, NLEV, nt)).astype(dtype) for _ in range(2)]
        labels = (np.arange(nt) % 3).astype(np.int32)
        labels[4] = -1
        w = rng.uniform(0.5, 2.0, nt)
        w[6] = 0.0                                          # labels[6] == 0
        y = [v.copy() for v in x]
        y[0][9, 0, 4] = np.nan                              # left out
        y[1][11, 1, 6] = np.nan                             # weight 0
        y[0][12, 2, 6] = np.inf
        for common in (True, False):
            a0, w0, c0, _ = mgsum(x, labels, 3, w, common=common)
            a1, w1, c1, _ = mgsum(y, labels, 3, w, common=common)
            for p, q in zip(a0 + w0, a1 + w1):
                assert p.tobytes() == q.tobytes() and np.all(np.isfinite(q))       # w = 0: the sums keep their bits
            for f, (p, q) in enumerate(zip(c0, c1)):                               # ... and the counts lose the time
                d = p - q
                hit = np.zeros_like(d, dtype=bool)
                if common or f == 1:
                    hit[11, 1, 0] = True
                if common or f == 0:
                    hit[12, 2, 0] = True
                assert np.all(d[hit] == 1) and np.all(d[~hit] == 0), (nt, common, f)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_nan_in_one_field_drops_the_time_from_all_under_the_common_mask_only(dtype):
    for nt in (30, switch(dtype) + 1):
        rng = np.random.default_rng(nt)
        x = [rng.standard_normal((NCOL, NLEV, nt)).astype(dtype) for _ in range(4)]
        labels, w = (np.arange(nt) % 2).astype(np.int32), rng.uniform(0.5, 2.0, nt)
        y = [v.copy() for v in x]
        y[2][5, 1, 8] = np.nan                              # group 0
        a0, w0, c0, _ = mgsum(x, labels, 2, w, common=True)
        a1, w1, c1, _ = mgsum(y, labels, 2, w, common=True)
        cut = [v.copy() for v in x]
        for v in cut:
            v[5, 1, 8] = np.nan                             # the same time missing in every field
        a2, w2, c2, _ = mgsum(cut, labels, 2, w, common=True)
        for p, q in zip(a1 + w1 + c1, a2 + w2 + c2):
            assert p.tobytes() == q.tobytes()
        assert c0[0][5, 1, 0] - c1[0][5, 1, 0] == 1 and all(a0[f][5, 1, 0] != a1[f][5, 1, 0] for f in range(4))
        assert w0[0][5, 1, 0] != w1[0][5, 1, 0]
        # own masks: only field 2 loses the time, and a field's results do not depend on what else the call carries
        b0, v0, d0, _ = mgsum(x, labels, 2, w, common=False)
        b1, v1, d1, _ = mgsum(y, labels, 2, w, common=False)
        for f in (0, 1, 3):
            assert b0[f].tobytes() == b1[f].tobytes() and v0[f].tobytes() == v1[f].tobytes() and d0[f].tobytes() == d1[f].tobytes()
        assert d0[2][5, 1, 0] - d1[2][5, 1, 0] == 1 and b0[2][5, 1, 0] != b1[2][5, 1, 0]
        (alone,), (va,), (da,), _ = mgsum([y[2]], labels, 2, w, common=False)
        assert alone.tobytes() == b1[2].tobytes() and va.tobytes() == v1[2].tobytes() and da.tobytes() == d1[2].tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_permuting_rows_permutes_the_bits(dtype):
    rows = NCOL * NLEV
    for nt in (30, 129, switch(dtype), 1000):
        rng = np.random.default_rng(nt)
        labels, w = make_labels("random", nt, 5, rng), make_weights(nt, rng)
        x = [v.reshape(rows, nt) for v in holes(4, nt, dtype, rng, labels)]
        perm = rng.permutation(rows)
        a = mgsum([v.reshape(NCOL, NLEV, nt) for v in x], labels, 5, w)[:3]
        for shape in ((NCOL, NLEV), (rows, 1), (1, rows)):
            b = mgsum([v[perm].reshape(shape + (nt,)) for v in x], labels, 5, w)[:3]
            for p, q in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]):
                assert p.reshape(rows, 5)[perm].tobytes() == q.tobytes(), (nt, shape)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_form_of_the_long_row_kernel_changes_no_bit(dtype):
    """The groups present pick the form (registers for at most 1 and at most 4, LDS beyond, in batches where one wave's
    image does not hold them all); a (row, group) keeps its bits while more of the other times, left out at first, are
    given to further groups.  Batched against unbatched: 8 fields with one mask under the common mask (12 groups per
    pass) against the same fields in own-mask mode (42 per pass)."""
    from pytemdiags_amd import _mgclim
    nt = switch(dtype) + 41
    rng = np.random.default_rng(8)
    w = make_weights(nt, rng)
    base = rng.integers(0, 30, nt).astype(np.int32)
    x = holes(4, nt, dtype, rng)
    got = {}
    for present in (1, 4, 5, 30):
        labels = np.where(base < present, base, -1).astype(np.int32)
        assert np.unique(labels[labels >= 0]).size == present
        a, ws, c, _ = mgsum(x, labels, 30, w)
        got[present] = np.stack(a + ws + c)
    assert [_mgclim.bound(n) for n in (1, 4, 5, 30)] == [1, 4, 64, 64]
    assert _mgclim.shape(111, nt, np.dtype(dtype).itemsize, 4, 30)["npass"] == 2
    for small, big in ((1, 4), (4, 5), (5, 30)):
        assert got[small][..., :small].tobytes() == got[big][..., :small].tobytes(), (small, big)
    hole = ~np.isfinite(x[0])
    same = [np.where(hole, np.nan, rng.standard_normal(hole.shape)).astype(dtype) for _ in range(8)]
    assert _mgclim.shape(111, nt, np.dtype(dtype).itemsize, 8, 30)["npass"] == 3
    assert _mgclim.shape(111, nt, np.dtype(dtype).itemsize, 1, 30)["npass"] == 1
    a, ws, c, _ = mgsum(same, base, 30, w, common=True)
    b, vs, d, _ = mgsum(same, base, 30, w, common=False)
    for f in range(8):
        assert a[f].tobytes() == b[f].tobytes() and ws[0].tobytes() == vs[f].tobytes() and c[0].tobytes() == d[f].tobytes()


@pytest.mark.parametrize("common", [True, False])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_blocks_accumulate_and_absent_groups_keep_their_bits(dtype, common):
    for ntr in (30, 2 * switch(dtype) + 90):
        rng = np.random.default_rng(ntr)
        ng = 12
        labels = ((np.arange(ntr) * 9) // ntr).astype(np.int32)          # groups 0..8 in runs; 9, 10, 11 never occur
        labels[ntr // 2] = -1
        w = make_weights(ntr, rng)
        x = holes(2, ntr, dtype, rng, labels)
        whole = mgsum(x, labels, ng, w, common=common)[:3]
        again = mgsum(x, labels, ng, w, common=common)[:3]
        for p, q in zip(whole[0] + whole[1] + whole[2], again[0] + again[1] + again[2]):
            assert p.tobytes() == q.tobytes()                             # repeated calls
            assert np.all(p[..., 9:] == 0)                                # absent: zero without the flag
        cuts = (0, ntr // 3, ntr // 3 + switch(dtype) // 2 + 1 if ntr > 100 else 2 * ntr // 3, ntr)
        sets = None
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            a, ws, c, sets = mgsum([v[..., b0:b1] for v in x], labels, ng, w, t0=b0, common=common, accumulate=sets is not None,
                                   into=sets)
        ok = masks(x, common)
        for f in range(2):
            _, tol = reference(np.where(ok[f], x[f], 0).astype(np.float64), labels, ng, w)
            assert np.all(np.abs(a[f] - whole[0][f]) <= tol), (ntr, f)
        for f in range(len(ws)):
            _, tol = reference(ok[f].astype(np.float64), labels, ng, w)
            assert np.all(np.abs(ws[f] - whole[1][f]) <= tol)
            assert np.array_equal(c[f], whole[2][f])                      # exact
        # under the flag an absent group is neither read nor written: the last block holds the groups 5.. only
        pre = rng.standard_normal((NCOL, NLEV, ng)) * 1e3
        b0 = cuts[2]
        absent = [g for g in range(ng) if not np.any(labels[b0:] == g)]
        assert len(absent) >= 4
        a, ws, c, _ = mgsum([v[..., b0:] for v in x], labels, ng, w, t0=b0, common=common, accumulate=True, prefill=pre)
        for p in a + ws + c:
            assert p[..., absent].tobytes() == pre[..., absent].tobytes()
        fresh = mgsum([v[..., b0:] for v in x], labels, ng, w, t0=b0, common=common)[:3]
        there = [g for g in range(ng) if g not in absent]
        for p, q in zip(a + ws + c, fresh[0] + fresh[1] + fresh[2]):
            assert p[..., there].tobytes() == (pre[..., there] + q[..., there]).tobytes()      # one further rounding
            assert np.all(q[..., absent] == 0)
        # a block whose labels are all -1
        none = np.full(ntr, -1, dtype=np.int32)
        z = mgsum(x, none, ng, None, common=common)[:3]
        assert all(np.all(p == 0) for p in z[0] + z[1] + z[2])
        kept = mgsum(x, none, ng, None, common=common, accumulate=True, prefill=pre)[:3]
        assert all(p.tobytes() == pre.tobytes() for p in kept[0] + kept[1] + kept[2])


def test_overlap_and_misalignment_are_refused_with_real_pointers_and_nothing_is_written():
    from pytemdiags_amd import _mgclim
    lib = _mgclim.load()
    ncol, nlev, nt, ng = 4, 3, 5, 2
    src = torch.zeros(ncol * nlev * nt + 8, dtype=torch.float64, device=DEV)
    out = torch.full((3 * ncol * nlev * ng + 16,), CANARY, dtype=torch.float64, device=DEV)
    lab = (C.c_int32 * 5)(0, 1, -1, 1, 0)
    m = ncol * nlev * ng * 8

    def call(s, a, w, c, flags=_mgclim.COMMON_MASK):
        one = lambda p: (C.c_void_p * 1)(p)
        return lib.temxw_time_sum_groups_valid(0, 1, one(s), 0, one(a), one(w), one(c), ncol, nlev, nt, nt, 0, ng, lab, None,
                                               flags, None)
    s, o = src.data_ptr(), out.data_ptr()
    err = lib.temx_last_error
    assert call(s, s + 8, o, o + m) == -1 and b"acc 0 overlaps src 0" in err()
    assert call(s, o, s + ncol * nlev * nt * 8 - 8, o + m) == -1 and b"wsum 0 overlaps src 0" in err()
    assert call(s, o, o + m, s) == -1 and b"cnt 0 overlaps src 0" in err()
    assert call(s, o, o + m - 8, o + 2 * m) == -1 and b"wsum 0 overlaps acc 0" in err()
    assert call(s, o, o + m, o + 8) == -1 and b"cnt 0 overlaps acc 0" in err()
    assert call(s, o, o + m, o + 2 * m - 8) == -1 and b"wsum 0 overlaps cnt 0" in err()
    assert call(s + 4, o, o + m, o + 2 * m) == -1 and b"aligned" in err()
    assert call(s, o + 4, o + m, o + 2 * m) == -1 and b"aligned" in err()
    assert call(s, o, o + m + 4, o + 2 * m) == -1 and b"wsum 0 is not aligned" in err()
    assert call(s, o, o + m, o + 2 * m + 4) == -1 and b"cnt 0 is not aligned" in err()
    assert call(s, o, None, o + 2 * m) == -1 and b"wsum 0 is null" in err()
    assert call(s, o, o + m, None) == -1 and b"cnt 0 is null" in err()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == CANARY) and not src.any()
    assert call(s, o, o + m, o + 2 * m) == 0                        # touching is fine
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[:ncol * nlev * ng] == 0) and np.all(got[m // 8:2 * m // 8].reshape(-1, 2) == [2, 2])
    assert np.all(got[2 * m // 8:3 * m // 8].reshape(-1, 2) == [2, 2]) and np.all(got[3 * m // 8:] == CANARY)
