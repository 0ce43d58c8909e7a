"""temxl_to_engine (include/temx_layout.h) on the GPU: time-major [nt][nlev][ncol] -> engine layout [ncol][nlev][ntb].

The kernel is compared bit for bit against ``src[t0:t0+ntb].permute(2, 1, 0)`` (plus flip or cast) through integer
views, so NaN payloads and -0.0 count.  Every destination is a slice out of the middle of a larger tensor filled with a
sentinel, and both guard regions must still hold the sentinel after the call.  The shapes cross every path of the
tile choice: windows that move whole with several levels per tile (ntb 1, 7, 33), whole over 32 columns (ntb 70 in
fp64), in chunks (ntb 70 needs no chunks in fp32; 130 and 300 do), and tails in ncol, nlev and ntb."""
import ctypes as C
import itertools

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
GUARD = 257                       # elements on either side of a destination (odd: dst is aligned to its element only)
SENTINEL = 12345.678
IVIEW = {torch.float64: torch.int64, torch.float32: torch.int32}
SPECIAL = {torch.float64: [0x7FF0000000000001, 0x7FF8000000ABCDEF, -0x8000000000000000, 0x7FF0000000000000,
                           -0x000FFFFFFFFFFFFF, 1],
           torch.float32: [0x7F800001, 0x7FC0ABCD, -0x80000000, 0x7F800000, -0x007FFFFF, 1]}
QUIET = {torch.float32: [0x7FC0ABCD, -0x80000000, 0x7F800000, -0x003FFFFF]}     # what a widening cast carries exactly


def _source(shape, dtype, gen, widened):
    """Random values with special bit patterns sprinkled in (signalling NaNs only where the move is a bit copy)."""
    s = torch.randn(shape, dtype=dtype, device=DEV, generator=gen)
    flat = s.view(IVIEW[dtype]).reshape(-1)
    pats = QUIET[dtype] if widened else SPECIAL[dtype]
    idx = torch.randint(0, flat.numel(), (len(pats),), device=DEV, generator=gen)
    flat[idx] = torch.tensor(pats, dtype=IVIEW[dtype], device=DEV)
    return s


def _expected_bits(s, t0, ntb, flip, dtype):
    w = s[t0:t0 + ntb]
    if s.dtype == dtype:
        w = w.view(IVIEW[dtype])                       # a bit copy
    else:
        w = w.to(dtype).view(IVIEW[dtype])             # fp32 -> fp64 widens
    w = w.permute(2, 1, 0)
    return (torch.flip(w, dims=(1,)) if flip else w).contiguous()


def _guarded(n, dtype):
    big = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return big, big[GUARD:GUARD + n]


def _guards_hold(big, n):
    ref = torch.full((GUARD,), SENTINEL, dtype=big.dtype, device=DEV).view(IVIEW[big.dtype])
    v = big.view(IVIEW[big.dtype])
    return torch.equal(v[:GUARD], ref) and torch.equal(v[GUARD + n:], ref)


def _dtypes(nf, mode):
    if mode == "f32":
        return [torch.float32] * nf, torch.float32
    # mixed sources widening to fp64: the first stays fp64, then alternating
    return [torch.float64 if f % 2 == 0 else torch.float32 for f in range(nf)], torch.float64


def _check(ncol, nlev, ntb, t0, nf, mode, flip, gen, nt_extra=5):
    from pytemdiags_amd.layout import to_engine_layout
    sdt, ddt = _dtypes(nf, mode)
    nt_src = ntb + nt_extra
    srcs = [_source((nt_src, nlev, ncol), dt, gen, widened=dt != ddt) for dt in sdt]
    n = ncol * nlev * ntb
    held = [_guarded(n, ddt) for _ in range(nf)]
    outs = to_engine_layout(srcs, t0=t0, ntb=ntb, flip_lev=flip, dtype=ddt,
                            out=[d.view(ncol, nlev, ntb) for _, d in held])
    for f in range(nf):
        want = _expected_bits(srcs[f], t0, ntb, flip, ddt)
        tag = (ncol, nlev, ntb, t0, nf, mode, flip, f)
        assert torch.equal(outs[f].view(IVIEW[ddt]), want), tag
        assert _guards_hold(held[f][0], n), tag


@pytest.mark.parametrize("ncol", [1, 37, 64, 866, 1025])
def test_to_engine_matches_permute_bit_for_bit_and_stays_in_bounds(ncol):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1000 + ncol)
    for nlev, ntb, t0, nf, mode, flip in itertools.product((1, 2, 9), (1, 7, 33, 70), (0, 5), (1, 5, 8),
                                                           ("mixed", "f32"), (False, True)):
        _check(ncol, nlev, ntb, t0, nf, mode, flip, gen)


@pytest.mark.parametrize("ntb,mode", [(130, "mixed"), (300, "mixed"), (300, "f32"), (64, "mixed"), (128, "f32")])
def test_to_engine_long_windows_move_in_chunks(ntb, mode):
    """Windows past twice the tile's rows (128 fp64, 256 fp32) are cut into chunks of 64 / 128 times, one level per
    tile; 64 and 128 sit on the thresholds."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(ntb)
    for ncol, nlev, flip in ((37, 2, True), (130, 3, False)):
        _check(ncol, nlev, ntb, 3, 2, mode, flip, gen)


def test_to_engine_defaults_allocate_and_pick_the_dtype():
    from pytemdiags_amd.layout import to_engine_layout
    a = torch.randn((6, 4, 50), dtype=torch.float32, device=DEV)
    b = torch.randn((6, 4, 50), dtype=torch.float64, device=DEV)
    o32, = to_engine_layout(a)
    assert o32.dtype == torch.float32 and tuple(o32.shape) == (50, 4, 6) and torch.equal(o32, a.permute(2, 1, 0))
    oa, ob = to_engine_layout([a, b], t0=2)
    assert oa.dtype == ob.dtype == torch.float64 and tuple(oa.shape) == (50, 4, 4)
    assert torch.equal(oa, a[2:].permute(2, 1, 0).double()) and torch.equal(ob, b[2:].permute(2, 1, 0))
    with pytest.raises(ValueError):
        to_engine_layout([a.permute(2, 1, 0)])                     # not contiguous
    with pytest.raises(ValueError):
        to_engine_layout([b], dtype=torch.float16)
    with pytest.raises(ValueError):
        to_engine_layout([a], t0=4, ntb=3)


# ---- offsets beyond 32 bits --------------------------------------------------------------------------------------
def _needs_24gb():
    free, _ = torch.cuda.mem_get_info()
    if free < 24e9:
        pytest.skip("needs 24 GB of free device memory")


def test_source_offsets_beyond_32_bits():
    """One fp32 source of 1 048 579 x 8 x 130 elements (more than 2^32 bytes), window t0 = 126, ntb = 4: only the
    window is filled, and compared against the small permuted window."""
    from pytemdiags_amd.layout import to_engine_layout
    _needs_24gb()
    ncol, nlev, nt, t0, ntb = 1048579, 8, 130, 126, 4
    src = torch.empty((nt, nlev, ncol), dtype=torch.float32, device=DEV)
    assert src.numel() * 4 > 2 ** 32
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    src[t0:] = torch.randn((ntb, nlev, ncol), dtype=torch.float32, device=DEV, generator=gen)
    n = ncol * nlev * ntb
    big, d = _guarded(n, torch.float32)
    out, = to_engine_layout([src], t0=t0, ntb=ntb, out=[d.view(ncol, nlev, ntb)])
    want = src[t0:].view(torch.int32).permute(2, 1, 0).contiguous()
    assert torch.equal(out.view(torch.int32), want)
    assert _guards_hold(big, n)


def test_destination_offsets_beyond_32_bits():
    """One fp64 destination above 2^32 bytes (ncol 1 048 579, nlev 8, ntb 65), checked on the first and last 1000
    columns directly against the source."""
    from pytemdiags_amd.layout import to_engine_layout
    _needs_24gb()
    ncol, nlev, ntb = 1048579, 8, 65
    gen = torch.Generator(device=DEV)
    gen.manual_seed(6)
    src = torch.randn((ntb, nlev, ncol), dtype=torch.float64, device=DEV, generator=gen)
    n = ncol * nlev * ntb
    assert n * 8 > 2 ** 32
    big, d = _guarded(n, torch.float64)
    out, = to_engine_layout([src], out=[d.view(ncol, nlev, ntb)])
    for sl in (slice(0, 1000), slice(ncol - 1000, ncol)):
        want = src[:, :, sl].view(torch.int64).permute(2, 1, 0).contiguous()
        assert torch.equal(out[sl].view(torch.int64), want)
    assert _guards_hold(big, n)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_every_einval_case_is_refused_and_dst_stays_untouched():
    from pytemdiags_amd import _layout
    lib = _layout.load()
    ncol, nlev, nt_src, ntb = 40, 3, 9, 4
    n = ncol * nlev * ntb
    s64 = [torch.randn((nt_src, nlev, ncol), dtype=torch.float64, device=DEV) for _ in range(2)]
    s32 = torch.randn((nt_src, nlev, ncol), dtype=torch.float32, device=DEV)
    held = [_guarded(n, torch.float64) for _ in range(2)]
    torch.cuda.synchronize()
    F64, F32 = _layout.F64, _layout.F32

    def vps(ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def ints(v):
        return (C.c_int * len(v))(*v)
    good = dict(nf=2, src=vps([s.data_ptr() for s in s64]), sdt=ints([F64, F64]),
                dst=vps([d.data_ptr() for _, d in held]), ddt=F64, ncol=ncol, nlev=nlev, nt_src=nt_src, t0=2, ntb=ntb,
                flags=0)

    def refused(names, **kw):
        a = dict(good, **kw)
        rc = lib.temxl_to_engine(0, a["nf"], a["src"], a["sdt"], a["dst"], a["ddt"], a["ncol"], a["nlev"], a["nt_src"],
                                 a["t0"], a["ntb"], a["flags"], None)
        msg = lib.temx_last_error().decode()
        assert rc == -1, (kw, rc, msg)
        assert any(w in msg for w in names), (kw, msg)

    refused(["nf"], nf=0)
    refused(["nf"], nf=_layout.NF_MAX + 1)
    refused(["src_host"], src=None)
    refused(["src_dtype_host"], sdt=None)
    refused(["dst_host"], dst=None)
    refused(["src 1"], src=vps([s64[0].data_ptr(), None]))
    refused(["dst 0"], dst=vps([None, held[1][1].data_ptr()]))
    refused(["ncol"], ncol=0)
    refused(["nlev"], nlev=0)
    refused(["nt_src"], nt_src=0)
    refused(["ntb"], ntb=0)
    refused(["t0"], t0=-1)
    refused(["t0 + ntb", "nt_src"], t0=6)                                    # 6 + 4 > 9
    refused(["t0 + ntb", "nt_src"], ntb=nt_src + 1, t0=0)
    refused(["flags"], flags=2)
    refused(["flags"], flags=-1)
    refused(["src_dtype 1"], sdt=ints([F64, 7]))
    refused(["dst_dtype"], ddt=5)
    refused(["src_dtype 0"], ddt=F32)                                         # fp64 -> fp32 narrows
    refused(["src 0", "aligned"], src=vps([s64[0].data_ptr() + 4, s64[1].data_ptr()]))
    refused(["src 1", "aligned"], src=vps([s64[0].data_ptr(), s32.data_ptr() + 2]), sdt=ints([F64, F32]))
    refused(["dst 1", "aligned"], dst=vps([held[0][1].data_ptr(), held[1][1].data_ptr() + 4]))
    refused(["dst 0 overlaps src 1"], dst=vps([s64[1].data_ptr() + 8 * 5, held[1][1].data_ptr()]))
    refused(["dst 1 overlaps src 0"], dst=vps([held[0][1].data_ptr(), s64[0].data_ptr() + 8 * (s64[0].numel() - 1)]))
    refused(["dst 1 overlaps dst 0"], dst=vps([held[0][1].data_ptr(), held[0][1].data_ptr() + 8 * (n - 1)]))
    torch.cuda.synchronize()
    sent = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    for big, _ in held:
        assert torch.equal(big, sent)                                         # no refused call wrote anything
    # and the well-formed call goes through
    a = good
    assert lib.temxl_to_engine(0, a["nf"], a["src"], a["sdt"], a["dst"], a["ddt"], ncol, nlev, nt_src, 2, ntb, 1, None) == 0
    torch.cuda.synchronize()
    for (big, d), s in zip(held, s64):
        assert torch.equal(d.view(ncol, nlev, ntb), torch.flip(s[2:6].permute(2, 1, 0), dims=(1,)))
        assert _guards_hold(big, n)
