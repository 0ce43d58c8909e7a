"""The time filter on the MI355X where tests/test_gpu_tfilt.py does not reach: the cuts that no call of it takes (fp64
``rpb = 16`` with several time tiles -- the cut of the ``nw = 121`` measurement -- fp64 ``rpb = 64``, fp32 ``rpb = 64`` and
``128``, row tails in fp32), the three ``NB = 3`` kernels, every remainder of the k loop with ``nw = 1`` among them, values
at the edges of the number formats, and global offsets beyond 2^31 elements.

Everything is held to the oracle of tests/test_gpu_tfilt.py, imported (``pool``, ``oracle``, ``record``, ``call``,
``Guarded``, ``check_against_oracle``, ``shape_of``, ``bits``): every output bit equal to the exact-fma chain in Fractions,
every guard word intact, ``rc == 0``.  Bits are compared, so ``-0.0`` against ``+0.0`` and a flushed subnormal both fail.
Every case first asserts, through ``temxf_filter_shape``, the cut it is aimed at (``expect_cut``): after a change of the cut
rule the case says that it no longer covers its cut instead of passing on another one.

The fp64 accumulator stays finite in every case by the choice of weights (the oracle raises OverflowError otherwise):
the band of large weights is ``4, -4, 4 ...`` for fp32 sources, whose largest value times 36 is far inside fp64, and
``2^-4, -2^-4 ...`` for fp64 sources, and the largest finite values of the edge pool stand 25 elements apart, more than the
nine weights of those bands.

Measured on the MI355X: every comparison in this file is of bits, and every one held; ``nw = 1`` is served.  The offsets
case ran (more than 40 GB free) and took 0.7 s; the slowest case is the ``nw = 121`` one, 0.9 s, most of it the oracle."""
import numpy as np
import pytest

import test_gpu_tfilt as tf
from test_gpu_tfilt import (DEV, GUARD, LMAX, POOL, bits, call, check_against_oracle, oracle, pool, record, row_ids, shape_of,
                            weights)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ESZ = {"f64": 8, "f32": 4, "x64": 8, "x32": 4}
F64, F32 = torch.float64, torch.float32


def expect_cut(rows, nt, nw, nb, src_esz, dst_esz, **want):
    """The cut of the launch, asserted before the launch: ``want`` names entries of ``temxf_filter_shape``."""
    sh = shape_of(rows, nt, nw, nb, src_esz, dst_esz)
    for name, v in want.items():
        assert sh[name] == v, "this case no longer covers %s = %d: rows %d nt %d nw %d esz %d give %r" % (
            name, v, rows, nt, nw, src_esz, sh)
    return sh


def dst_esz(dtype):
    return 4 if dtype == F32 else 8


# ---- 1. the cut of the nw = 121 measurement, and the two widths at which fp64 rows are given up -----------------------
def test_fp64_nw_121_sixteen_rows_by_128_one_two_and_three_tiles():
    nw, TT = 121, 128
    w = weights(nw, 2)
    for nto, ntile in ((TT, 1), (TT + 3, 2), (2 * TT + 1, 3)):
        nt = nto + nw - 1
        assert nt <= LMAX
        for rows in (1, 15, 17, 33):
            expect_cut(rows, nt, nw, 2, 8, 8, rpb=16, TT=TT, ntile=ntile)
            check_against_oracle(["f64"], rows, 1, nt, w, F64, "nw 121 nto %d rows %d" % (nto, rows))


@pytest.mark.parametrize("nw,rpb,TT", [(97, 16, 128), (193, 8, 256)])
def test_fp64_first_widths_that_give_up_rows(nw, rpb, TT):
    """temx_tfilt.h: 16 rows by 128 for fp64 sources with nw > 96, 8 rows by 256 with nw > 192; a row of fewer than 64
    outputs has fewer runs than lanes and takes twice as many rows again (the short record: 20 outputs in 24)."""
    w = weights(nw, 1)
    assert shape_of(10, nw - 2 + 4000, nw - 2)["rpb"] == 2 * rpb          # (the width before it still has the rows)
    nt = TT + 3 + nw - 1
    for rows in (rpb - 1, rpb + 1):
        expect_cut(rows, nt, nw, 1, 8, 8, rpb=rpb, TT=TT, ntile=2)
        check_against_oracle(["f64"], rows, 1, nt, w, F64, "nw %d long rows %d" % (nw, rows))
    nt = 20 + nw - 1
    expect_cut(2 * rpb + 1, nt, nw, 1, 8, 8, rpb=2 * rpb, TT=24, ntile=1)
    check_against_oracle(["f64"], 2 * rpb + 1, 1, nt, w, F64, "nw %d short" % nw)


# ---- 2. many rows per workgroup, both source types ---------------------------------------------------------------------
MANY = [("f64", 5, 21, 64, 24, F64), ("f64", 13, 42, 64, 32, F64),
        ("f32", 5, 14, 128, 16, F32), ("f32", 5, 14, 128, 16, F64), ("f32", 21, 36, 128, 16, F32), ("f32", 21, 36, 128, 16, F64),
        ("f32", 9, 40, 64, 32, F32), ("f32", 9, 40, 64, 32, F64), ("f32", 3, 4, 256, 8, F32), ("f32", 3, 4, 256, 8, F64)]


@pytest.mark.parametrize("kind,nw,nt,rpb,TT,out", MANY, ids=["%s-nw%d-nt%d-rpb%d-to%d" % (c[0], c[1], c[2], c[3], dst_esz(c[5]) * 8) for c in MANY])
def test_many_rows_per_workgroup_and_their_row_tails(kind, nw, nt, rpb, TT, out):
    """``rpb - 1``, ``rpb`` and ``rpb + 1`` rows, and ``3 rpb + 5``: a second and a fourth row block."""
    w = weights(nw, 2)
    for rows in (rpb - 1, rpb, rpb + 1, 3 * rpb + 5):
        expect_cut(rows, nt, nw, 2, ESZ[kind], dst_esz(out), rpb=rpb, TT=TT, ntile=1, grid=-(-rows // rpb))
        check_against_oracle([kind], rows, 1, nt, w, out, "%s nw %d rpb %d rows %d" % (kind, nw, rpb, rows))


def test_the_served_call_of_the_refusal_test_fp32_rpb_64():
    """The last call of ``test_refused_calls_leave_the_destinations_untouched``, which only asks for "not untouched"."""
    expect_cut(24, 40, 9, 2, 4, 4, rpb=64, TT=32, ntile=1, grid=1)
    check_against_oracle(["f32"], 12, 2, 40, weights(9, 2), F32, "12 x 2 x 40 fp32")


# ---- 3. the NB = 3 kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds,out,nt", [(["f64"], F64, 143), (["f32"], F64, 271), (["f32"], F32, 271), (["f64", "f32", "f64"], F64, 271)],
                         ids=["f64-to64", "f32-to64", "f32-to32", "mixed-to64"])
def test_three_bands(kinds, out, nt):
    """``tfilt_kernel<T, D, 3>`` for the three (T, D): distinct weights per band, 33 rows, ``nto = TT + 3`` (fp64: 128, fp32:
    256); the mixed call runs the fp64 and the fp32 launch of one call (fp64 then has ``2 TT + 3``)."""
    nw, w = 13, weights(13, 3)
    assert len({w[b].tobytes() for b in range(3)}) == 3
    for esz in sorted({ESZ[k] for k in kinds}):
        TT = 128 if esz == 8 else 256
        expect_cut(33, nt, nw, 3, esz, dst_esz(out), rpb=32, TT=TT, ntile=-(-(nt - nw + 1) // TT), grid=2 * -(-(nt - nw + 1) // TT))
        assert (nt - nw + 1) % TT == 3
    check_against_oracle(kinds, 11, 3, nt, w, out, "nb 3 %s" % "+".join(kinds))


# ---- 4. every remainder of the k loop ----------------------------------------------------------------------------------
TAILS = {1: (0, 1), 5: (0, 5), 7: (0, 7), 13: (1, 5), 15: (1, 7), 17: (2, 1), 21: (2, 5)}      # nw: (trips, remainder)


@pytest.mark.parametrize("nw", sorted(TAILS))
def test_k_loop_trips_and_remainders(nw):
    """The k loop is unrolled by R = 8 with a remainder block: zero, one and two trips, remainders 1, 5 and 7; one
    output, nine, and a tile and three."""
    assert (nw // 8, nw % 8) == TAILS[nw] and shape_of(10, nw + 4000, nw)["R"] == 8
    w = weights(nw, 1)
    TT = 128
    expect_cut(33, TT + 3 + nw - 1, nw, 1, 8, 8, rpb=32, TT=TT, ntile=2)
    check_against_oracle(["f64"], 33, 1, TT + 3 + nw - 1, w, F64, "nw %d nto TT + 3" % nw)
    for nto, rpb in ((1, 256 if nw < 9 else 128), (9, 128)):
        expect_cut(rpb + 1, nto + nw - 1, nw, 1, 8, 8, rpb=rpb, TT=-(-nto // 8) * 8, ntile=1, grid=2)
        check_against_oracle(["f64"], rpb + 1, 1, nto + nw - 1, w, F64, "nw %d nto %d" % (nw, nto))


@pytest.mark.parametrize("kind,out", [("x64", F64), ("f64", F64), ("x32", F32), ("x32", F64), ("f32", F64)],
                         ids=["x64", "f64", "x32-to32", "x32-to64", "f32-to64"])
def test_one_weight_of_1_copies_the_record(kind, out):
    """``nw = 1`` with ``w = [1.0]``: the output is the input bit for bit -- subnormals, the largest values, and an fp32
    subnormal as its exact fp64 value -- except that ``-0.0`` comes out as ``+0.0``, because the chain starts from
    ``+0.0``.  Also with ``nt = 1``."""
    w = np.ones((1, 1))
    for ncol, nlev, nt in ((33, 2, 400), (300, 1, 1)):
        x = record(kind, ncol, nlev, nt)
        rc, dst = call([x], w, out)
        assert rc == 0 and dst[0][0].guards_intact()
        src = pool(kind)[row_ids(ncol * nlev), :nt]
        want = (src.astype(np.float64) + 0.0).astype(np.float32 if out == F32 else np.float64)
        got = dst[0][0].values((ncol * nlev, nt))
        if kind[0] == "x" and nt > 1:
            assert np.signbit(src[src == 0]).any() and not np.signbit(want[want == 0]).any()
            assert ((src != 0) & (np.abs(src) < np.finfo(src.dtype).tiny)).any()
        assert (bits(got) == bits(want)).all(), (kind, nt, np.argwhere(bits(got) != bits(want))[:4].tolist())
        check_against_oracle([kind], ncol, nlev, nt, w, out, "nw 1 %s nt %d" % (kind, nt))


# ---- 5. values ---------------------------------------------------------------------------------------------------------
def edge_weights(kind):
    """Two bands of nine weights: ``lanczos(9, high=0.2)``, a high-pass whose weights sum to 0, and weights of one large
    magnitude and alternating sign -- 4 for fp32 sources, so that fp32 results pass FLT_MAX, and 2^-4 for fp64 sources,
    so that the fp64 accumulator stays finite next to the largest fp64 value."""
    from pytemdiags_amd.timebands import lanczos
    alt = (4.0 if kind == "x32" else 2.0 ** -4) * (-1.0) ** np.arange(9)
    return np.ascontiguousarray(np.stack([lanczos(9, high=0.2), alt]))


def edge_expectation(kind, out):
    """(weights, expected outputs ``[2][POOL][LMAX - 8]``) of the hand-placed pool, with what they must hold asserted on
    the oracle alone (no device): results below the smallest normal number of the source type and exact zeros; negative zeros where the
    destination can receive one (an fp64 chain that starts from +0.0 reaches -0.0 only through an underflow, which fp32
    sources cannot cause: there the zeros are all positive); for an fp32 destination both infinities; for fp32 into
    fp64 values below the smallest fp32 subnormal, which exist only if the source was widened exactly, and 4 FLT_MAX."""
    w = edge_weights(kind)
    assert abs(float(np.sum(w[0]))) < 1e-15
    nto = LMAX - 8
    out32 = out == F32
    want = np.stack([[oracle(kind, p, w[b], nto, out32) for p in range(POOL)] for b in range(2)])
    tiny = np.finfo(pool(kind).dtype).tiny
    zeros = want[want == 0]
    assert ((want != 0) & (np.abs(want) < tiny)).any() and zeros.size > 10 and not np.isnan(want).any()
    assert np.signbit(zeros).any() != ((kind, out) == ("x32", F64)) and not np.signbit(zeros).all()
    if out32:
        assert np.isposinf(want).any() and np.isneginf(want).any()
    else:
        assert np.isfinite(want).all()
    if (kind, out) == ("x32", F64):
        assert ((want != 0) & (np.abs(want) < 2.0 ** -149)).any() and np.abs(want).max() == 4.0 * float(np.finfo(np.float32).max)
    return w, want


@pytest.mark.parametrize("kind,out", [("x64", F64), ("x32", F32), ("x32", F64)], ids=["x64", "x32-to32", "x32-to64"])
def test_subnormals_signed_zeros_largest_values_and_cancelling_weights(kind, out):
    """The hand-placed pool under a high-pass and under large alternating weights, 40 rows by the whole pool length;
    ``edge_expectation`` says what the expected outputs hold."""
    w, _ = edge_expectation(kind, out)
    nt, nto = LMAX, LMAX - 8
    expect_cut(40, nt, 9, 2, ESZ[kind], dst_esz(out), rpb=32, ntile=-(-nto // (128 if kind == "x64" else 256)))
    check_against_oracle([kind], 20, 2, nt, w, out, "values %s" % kind)


# ---- 6. offsets beyond 2^31 elements -----------------------------------------------------------------------------------
def test_row_blocks_beyond_2_to_the_31_elements_fp32():
    """fp32 to fp32, ``nw = 3``, ``nt = 4099`` (32 rows by 256, 17 tiles, the last of one output) and 524 000 rows: the
    smallest count at which two whole row blocks start at or beyond element 2^31 of the source (8.6 GB of source; the
    destination, two elements shorter per row, ends 0.03 % below 2^31 elements); a source offset kept in 32 bits goes
    wrong in them.  The record is three pool rows indexed on the device, the expected rows (3 x 4097, from the Fraction oracle) are indexed the same way and compared on the device as int32
    in chunks of rows; the guards and three row blocks -- the first, the one that straddles 2^31 and the last -- are
    compared on the host as well.  Not 2^32: 35 GB on a shared card is too much for what one more bit would add -- the
    offsets are int64_t or they are not.  Skipped only with less than 40 GB free."""
    free = torch.cuda.mem_get_info()[0]
    if free < 40e9:
        pytest.skip("%.1f GB of device memory free, the case is run with 40 GB or more" % (free / 1e9))
    nw, nt, rpb = 3, 4099, 32
    nto = nt - nw + 1
    first = -(-2 ** 31 // (rpb * nt))                       # the first row block that starts at or beyond element 2^31
    rows = (first + 2) * rpb
    assert rows == 524000 and (first - 1) * rpb * nt < 2 ** 31 <= first * rpb * nt and rows * nt > 2 ** 31
    expect_cut(rows, nt, nw, 1, 4, 4, rpb=rpb, TT=256, ntile=17, grid=17 * (first + 2))
    assert nto - 16 * 256 == 1
    if "o32" not in tf._pool:
        rng = np.random.default_rng(31)
        a = (rng.standard_normal((POOL, nt)) * 10.0 ** rng.integers(-3, 4, size=(POOL, nt))).astype(np.float32)
        a.setflags(write=False)
        tf._pool["o32"] = a
    w = weights(nw, 1)
    want = np.stack([oracle("o32", p, w[0], nto, True) for p in range(POOL)])
    ids = row_ids(rows)
    ids_d = torch.tensor(ids, device=DEV)
    x = torch.tensor(pool("o32"), device=DEV)[ids_d].view(rows, 1, nt)
    assert x.numel() > 2 ** 31 and x.is_contiguous()
    rc, dst = call([x], w, F32)
    assert rc == 0
    g = dst[0][0]
    sent = np.float32(g.sent)
    assert np.all(g.buf[:GUARD].cpu().numpy() == sent) and np.all(g.buf[GUARD + g.n:].cpu().numpy() == sent)
    got = g.buf[GUARD:GUARD + g.n].view(rows, nto).view(torch.int32)
    want_d = torch.tensor(bits(want), device=DEV)
    step = 65536
    for r0 in range(0, rows, step):
        if not torch.equal(got[r0:r0 + step], want_d[ids_d[r0:r0 + step]]):
            bad = (got[r0:r0 + step] != want_d[ids_d[r0:r0 + step]]).nonzero()
            raise AssertionError("rows from %d: %d outputs differ, the first at %r" % (r0, bad.shape[0], bad[0].tolist()))
    for b in (0, first - 1, first + 1):
        blk = got[b * rpb:(b + 1) * rpb].cpu().numpy()
        assert np.array_equal(blk, bits(want)[ids[b * rpb:(b + 1) * rpb]]), b
    del x, dst, g, got, want_d
    torch.cuda.empty_cache()
