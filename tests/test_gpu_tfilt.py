"""The time filter on the MI355X, the kernel alone (pytemdiags_amd/include/temx_tfilt.h, temxf_filter_time), bit for bit.

Oracle: the contract's own chain, ``acc = fma(w[b][k], x, acc)`` with k ascending from +0.0, with an exact fma built from
``fractions.Fraction`` (``float(Fraction(w) * Fraction(x) + Fraction(acc))`` is correctly rounded), and one rounding to
fp32 at the end for an fp32 destination.  It is evaluated once per row of a small pool of rows; the records of the tests
are made of those rows (a record of ``nt`` times holds their first ``nt`` elements), so an output is looked up, not
computed again -- which is the contract: the bits of an output depend on its window, the weights and the dtypes, not on
where the row lies, how long the record is or how the launch is cut.  The edges of the cut come from
``temxf_filter_shape``.

Two pools.  ``"f64"`` / ``"f32"``: random normal numbers between 1e-3 and 1e3.  ``"x64"`` / ``"x32"`` (``edge_pool``):
hand-placed values of the source type -- subnormals, signed zeros, the largest finite value and its negative, values
around the smallest normal number whose products with weights below 1 are subnormal, equal and opposite neighbours that
cancel exactly -- for tests/test_gpu_tfilt_edges.py.  ``exact_fma`` carries them: ``float(Fraction)`` is correctly rounded
into the subnormal range and keeps the sign of an underflow, an exact zero gets the sign IEEE 754 gives it under round to
nearest, and the one rounding to fp32 is ``np.float32(acc)``, which overflows to inf.  The fp64 accumulator itself must
stay finite (``float(Fraction)`` raises OverflowError otherwise): that is the caller's choice of weights, and the largest
finite values of the edge pool stand at least 20 elements apart for it."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
POOL, LMAX = 3, 800
GUARD = 64                                  # guard elements on either side of every destination
SENTINEL = {8: -6.02214076e23, 4: np.float32(-6.02214076e23)}
_pool, _oracle = {}, {}


def edge_pool(kind):
    """``[POOL][LMAX]`` hand-placed rows, float64 (``"x64"``) or float32 (``"x32"``), in stretches of 50 elements: (0) only
    values of at most four times the smallest normal number -- subnormals, both zeros, neighbours of the smallest normal
    -- so that whole windows of them give subnormal and underflowing sums; (1) moderate numbers with equal and opposite
    neighbours, both zeros among them; (2) a mixture of the two with the largest finite value, sign alternating, at every
    25th element, so that no window of fewer than 25 weights holds two of them; (3) runs of ten equal values of list
    (0), which weights that sum to 0 take to a sum far below the smallest subnormal, or to an exact zero.  Row p walks
    the lists with a step of its own (1, 5, 7: coprime to their lengths), so different neighbours meet in different
    rows."""
    t = np.float64 if kind == "x64" else np.float32
    fi = np.finfo(t)
    tiny, den, big, eps = float(fi.tiny), float(fi.smallest_subnormal), float(fi.max), float(fi.eps)
    small = [den, -den, 3 * den, tiny, -tiny, tiny - den, 1.5 * tiny, -1.5 * tiny, 0.0, -0.0, 2 * tiny, -(tiny + den), 5 * den,
             -0.0, 0.0, -3 * tiny]
    moderate = [1.5, 1.5, -1.5, -1.5, 0.0, -0.0, 3.25, -3.25, 1 + eps, -(1 + eps), 0.1, 0.1]
    a = np.zeros((POOL, LMAX), dtype=t)
    for p, step in enumerate((1, 5, 7)):
        for i in range(LMAX):
            seg = (i // 50) % 4
            v = small[i * step % 16] if seg == 0 or (seg == 2 and i % 2) else moderate[i * step % 12]
            if seg == 3:
                v = small[i // 10 * step % 16]
            if seg == 2 and i % 25 == 7 + p:
                v = big if (i // 25) % 2 else -big
            a[p, i] = v
    return a


def pool(kind):
    """``[POOL][LMAX]`` rows of mixed magnitude, float64 or float32 (built once, never written to); ``"x64"`` / ``"x32"``:
    the hand-placed rows of ``edge_pool``."""
    if kind not in _pool and kind in ("x64", "x32"):
        a = edge_pool(kind)
        a.setflags(write=False)
        _pool[kind] = a
    if kind not in _pool:
        rng = np.random.default_rng(11 if kind == "f64" else 12)
        a = rng.standard_normal((POOL, LMAX)) * 10.0 ** rng.integers(-3, 4, size=(POOL, LMAX))
        a = a.astype(np.float64 if kind == "f64" else np.float32)
        a.setflags(write=False)
        _pool[kind] = a
    return _pool[kind]


def weights(nw, nb):
    """``[nb][nw]`` distinct weights per band (seeded by the shape)."""
    rng = np.random.default_rng(1000 * nw + nb)
    return np.ascontiguousarray(rng.standard_normal((nb, nw)) / np.sqrt(nw))


def exact_fma(fw, fx, acc, w, x):
    """``fma(w, x, acc)`` of finite doubles, correctly rounded (``fw``, ``fx``: ``w`` and ``x`` as Fractions).  A sum that
    is not zero goes through ``float(Fraction)``: correctly rounded, subnormals included, and a result that underflows
    keeps its sign.  An exact zero is ``-0.0`` only where the product and the addend are both negative zeros, and ``+0.0``
    otherwise (round to nearest: ``x + (-x) = +0``, ``(+0) + (-0) = +0``)."""
    s = fw * fx + Fraction(acc)
    if s:
        return float(s)
    if acc == 0.0 and math.copysign(1.0, acc) < 0 and (w == 0.0 or x == 0.0) and math.copysign(1.0, w) * math.copysign(1.0, x) < 0:
        return -0.0
    return 0.0


def oracle(kind, p, w, nto, out32):
    """The first ``nto`` outputs of pool row ``p`` under the weights ``w`` ``[nw]``: exact fma chain in Fractions, one
    rounding to fp32 at the end for an fp32 destination (overflow to inf included)."""
    key = (kind, p, w.tobytes(), out32)
    have = _oracle.get(key, np.zeros(0))
    if have.size < nto:
        xs = [float(v) for v in pool(kind)[p]]
        ws = [float(v) for v in w]
        row = [Fraction(v) for v in xs]
        fw = [Fraction(v) for v in ws]
        out = list(have)
        for t in range(have.size, nto):
            acc = 0.0
            for k, wk in enumerate(fw):
                acc = exact_fma(wk, row[t + k], acc, ws[k], xs[t + k])
            with np.errstate(over="ignore"):
                out.append(np.float32(acc) if out32 else acc)
        have = np.array(out, dtype=np.float32 if out32 else np.float64)
        _oracle[key] = have
    return have[:nto]


def row_ids(rows):
    return (np.arange(rows) * 5 + 1) % POOL


def record(kind, ncol, nlev, nt):
    """A device tensor ``[ncol][nlev][nt]`` whose row r is the first nt elements of pool row ``row_ids[r]``."""
    a = pool(kind)[row_ids(ncol * nlev), :nt].reshape(ncol, nlev, nt)
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def shape_of(rows, nt, nw, nb=1, src_esz=8, dst_esz=8):
    from pytemdiags_amd import _tfilt
    return _tfilt.shape(rows, nt, nw, nb, src_esz, dst_esz)


class Guarded:
    """A destination ``[ncol][nlev][nto]`` inside a larger buffer filled with a sentinel."""

    def __init__(self, n, dtype):
        self.n = n
        self.sent = SENTINEL[torch.empty(0, dtype=dtype).element_size()]
        self.buf = torch.full((n + 2 * GUARD,), float(self.sent), dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:GUARD] == self.sent) and np.all(b[GUARD + self.n:] == self.sent))

    def untouched(self):
        return bool(np.all(self.buf.cpu().numpy() == self.sent))

    def values(self, shape):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().reshape(shape)


def call(fields, w, out_dtype, stream=None, **over):
    """temxf_filter_time on device tensors ``fields`` with host weights ``w`` ``[nb][nw]`` -> (rc, guarded destinations
    ``[nb][nf]``)."""
    from pytemdiags_amd import _tfilt
    from pytemdiags_amd.engine import _DT
    lib = _tfilt.load()
    ncol, nlev, nt = fields[0].shape
    nb, nw = w.shape
    nf = len(fields)
    wd = torch.tensor(w, device=DEV)
    dst = [[Guarded(ncol * nlev * (nt - nw + 1), out_dtype) for _ in range(nf)] for _ in range(nb)]
    a = dict(device=0, nf=nf, src=[x.data_ptr() for x in fields], dts=[_DT[x.dtype] for x in fields], nb=nb,
             dst=[g.ptr for band in dst for g in band], dd=_DT[out_dtype], ncol=ncol, nlev=nlev, nt=nt, nw=nw, wptr=wd.data_ptr(), flags=0)
    a.update(over)
    st = C.c_void_p((stream or torch.cuda.current_stream(DEV)).cuda_stream)
    if stream is not None:
        torch.cuda.synchronize()            # the buffers were filled on the current stream
    rc = lib.temxf_filter_time(a["device"], a["nf"], (C.c_void_p * len(a["src"]))(*a["src"]), (C.c_int * len(a["dts"]))(*a["dts"]),
                               a["nb"], (C.c_void_p * len(a["dst"]))(*a["dst"]), a["dd"], a["ncol"], a["nlev"], a["nt"], a["nw"],
                               C.c_void_p(a["wptr"]), a["flags"], st)
    torch.cuda.synchronize()
    return rc, dst


def check_against_oracle(kinds, ncol, nlev, nt, w, out_dtype, tag):
    """One call on a record per entry of ``kinds`` (``"f64"`` / ``"f32"``); every output against the oracle, every guard
    word intact."""
    fields = [record(k, ncol, nlev, nt) for k in kinds]
    rc, dst = call(fields, w, out_dtype)
    assert rc == 0, (tag, rc)
    nb, nw = w.shape
    nto = nt - nw + 1
    ids = row_ids(ncol * nlev)
    out32 = out_dtype == torch.float32
    for b in range(nb):
        for f, kind in enumerate(kinds):
            assert dst[b][f].guards_intact(), (tag, b, f)
            got = dst[b][f].values((ncol * nlev, nto))
            want = np.stack([oracle(kind, p, w[b], nto, out32) for p in range(POOL)])[ids]
            same = bits(got) == bits(want)
            assert same.all(), (tag, b, f, int((~same).sum()), np.argwhere(~same)[:4].tolist())


# ---- shapes against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [3, 31, 255])
def test_cut_edges_along_time_and_rows_fp64(nw):
    """``nt = nw`` (one output), ``nt = nw + 1``, ``nto`` of one time tile, one tile + 3 and two tiles + 1; 1, ``rpb - 1``
    and ``rpb + 1`` rows -- the edges as ``temxf_filter_shape`` gives them for each record."""
    w = weights(nw, 1)
    TT = shape_of(10, nw + 4000, nw)["TT"]
    assert TT + nw - 1 <= LMAX and 2 * TT + nw <= LMAX
    for nto in (1, 2, TT, TT + 3, 2 * TT + 1):
        nt = nto + nw - 1
        sh = shape_of(10, nt, nw)
        if nto >= TT:
            assert sh["TT"] == TT and sh["ntile"] == -(-nto // TT), sh
        rpb = sh["rpb"]
        for rows in sorted({1, max(rpb - 1, 1), rpb + 1}):
            assert shape_of(rows, nt, nw)["rpb"] == rpb
            check_against_oracle(["f64"], rows, 1, nt, w, torch.float64, "nw %d nto %d rows %d" % (nw, nto, rows))


def test_thousand_columns_three_levels_four_bands_eight_mixed_fields():
    """1000 columns x 3 levels, nw = 31, four bands of distinct weights, eight sources of mixed fp32 and fp64 -> fp64."""
    check_against_oracle(["f64", "f32", "f32", "f64", "f32", "f64", "f64", "f32"], 1000, 3, 100, weights(31, 4), torch.float64,
                         "1000 x 3, nb 4, nf 8")


@pytest.mark.parametrize("nb", [1, 4])
def test_fp32_destination_from_fp32_sources(nb):
    nw = 31
    TT = shape_of(10, nw + 4000, nw, nb, 4, 4)["TT"]
    for nto, rows in ((1, 300), (TT + 3, 33), (2 * TT + 1, 5)):
        check_against_oracle(["f32"] * (1 if nb == 4 else 2), rows, 1, nto + nw - 1, weights(nw, nb), torch.float32,
                             "fp32 nb %d nto %d" % (nb, nto))


def test_fp32_sources_widen_into_an_fp64_destination_nw_3_and_255():
    check_against_oracle(["f32"], 40, 2, 90, weights(3, 2), torch.float64, "fp32 -> fp64 nw 3")
    check_against_oracle(["f32"], 9, 1, 300, weights(255, 1), torch.float64, "fp32 -> fp64 nw 255")


# ---- properties ---------------------------------------------------------------------------------------------------------
def test_equal_rows_in_records_of_different_length_give_equal_bits():
    nw, w = 31, weights(31, 2)
    TT = shape_of(10, nw + 4000, nw)["TT"]
    short, long_ = 40 + nw - 1, 2 * TT + 1 + nw - 1            # one tile against three
    outs = {}
    for nt, (ncol, nlev) in ((short, (7, 3)), (long_, (70, 1))):
        rc, dst = call([record("f64", ncol, nlev, nt)], w, torch.float64)
        assert rc == 0
        outs[nt] = [dst[b][0].values((ncol * nlev, nt - nw + 1)) for b in range(2)]
    ids_s, ids_l = row_ids(21), row_ids(70)
    for b in range(2):
        for p in range(POOL):
            a = outs[short][b][ids_s == p]
            c = outs[long_][b][ids_l == p][:, :40]
            assert (bits(a) == bits(a[:1])).all() and (bits(c) == bits(c[:1])).all() and (bits(a[0]) == bits(c[0])).all(), (b, p)


@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_sources_off_a_16_byte_boundary_repeat_and_side_stream(kind):
    nw, w = 9, weights(9, 2)
    ncol, nlev, nt = 45, 2, 150
    x = record(kind, ncol, nlev, nt)
    odt = torch.float64 if kind == "f64" else torch.float32
    rc, d0 = call([x], w, odt)
    assert rc == 0
    ref = [d0[b][0].values((ncol * nlev, nt - nw + 1)) for b in range(2)]
    for off in (1, 3):                                          # elements past a 256-byte boundary
        buf = torch.empty(x.numel() + 8, dtype=x.dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        y = buf[off:off + x.numel()].view(ncol, nlev, nt)
        y.copy_(x)
        assert y.data_ptr() % 16 == off * x.element_size() % 16 != 0
        rc, d1 = call([y], w, odt)
        assert rc == 0
        for b in range(2):
            assert (bits(d1[b][0].values(ref[b].shape)) == bits(ref[b])).all(), (off, b)
    rc, d2 = call([x], w, odt)                                  # a repeated call
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    rc3, d3 = call([x], w, odt, stream=side)                    # a call on a side stream
    assert rc == 0 and rc3 == 0
    for b in range(2):
        assert (bits(d2[b][0].values(ref[b].shape)) == bits(ref[b])).all() and d3[b][0].guards_intact()
        assert (bits(d3[b][0].values(ref[b].shape)) == bits(ref[b])).all()


def test_a_nan_and_an_inf_stay_in_their_windows():
    nw, w = 31, weights(31, 2)
    ncol, nlev, nt = 40, 2, 200
    nto = nt - nw + 1
    x = record("f64", ncol, nlev, nt)
    rc, clean = call([x], w, torch.float64)
    y = x.clone()
    spots = {(3, 1, 0): float("nan"), (17, 0, 100): float("inf"), (39, 1, nt - 1): float("-inf"), (20, 0, 15): float("nan")}
    for (i, k, t), v in spots.items():
        y[i, k, t] = v
    rc2, dirty = call([y], w, torch.float64)
    assert rc == 0 and rc2 == 0
    touched = np.zeros((ncol, nlev, nto), dtype=bool)
    for (i, k, t) in spots:
        touched[i, k, max(t - nw + 1, 0):min(t, nto - 1) + 1] = True
    for b in range(2):
        a, d = clean[b][0].values((ncol, nlev, nto)), dirty[b][0].values((ncol, nlev, nto))
        assert dirty[b][0].guards_intact()
        assert not np.isfinite(d[touched]).any() and np.isfinite(a).all()
        assert (bits(d[~touched]) == bits(a[~touched])).all()


def test_refused_calls_leave_the_destinations_untouched():
    w = weights(9, 2)
    x64, x32 = record("f64", 12, 2, 40), record("f32", 12, 2, 40)
    n = 12 * 2 * 32
    spare = Guarded(n, torch.float64)
    cases = [dict(nw=8), dict(nt=8), dict(nb=5), dict(nf=0), dict(flags=2), dict(dts=[7]), dict(wptr=0), dict(ncol=0),
             dict(dd=1), dict(src=[x64.data_ptr() + 4])]
    for over in cases:
        rc, dst = call([x64], w, torch.float64, **over)
        assert rc == -1, over
        assert all(g.untouched() for band in dst for g in band), over
    rc, dst = call([x64], w, torch.float64, dst=[spare.ptr, spare.ptr + 8])       # the bands overlap each other
    assert rc == -1 and spare.untouched()
    rc, dst = call([x64], w, torch.float64, dst=[spare.ptr, x64.data_ptr() + 64])  # a band overlaps the source
    assert rc == -1 and spare.untouched() and (bits(x64.cpu().numpy()) == bits(record("f64", 12, 2, 40).cpu().numpy())).all()
    rc, dst = call([x32], w, torch.float32)                                        # and the call is served once it is right
    assert rc == 0 and all(g.guards_intact() and not g.untouched() for band in dst for g in band)
