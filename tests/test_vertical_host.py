"""Model levels to pressure levels, the part that needs no GPU: the numpy restatement of the contract of
include/temx_vert.h (``interp_ref``, which test_gpu_vertical.py compares the kernels against), the fixtures both
files share, self-checks of that reference, the validation errors raised before any device work, and the header,
the ctypes table and a plain-C consumer of the second header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 37 standard pressure levels [hPa]
PLEV37 = np.array([1, 2, 3, 5, 7, 10, 20, 30, 50, 70, 100, 125, 150, 175, 200, 225, 250, 300, 350, 400, 450, 500, 550,
                   600, 650, 700, 750, 775, 800, 825, 850, 875, 900, 925, 950, 975, 1000], dtype=np.float64)


def interp_ref(f, p, plev_pa, method="log", edge="nan", psurf=None):
    """The contract, per (column, time): np.interp over ln p or p inside [p_top, p_bot]; outside, NaN or (edge="hold")
    the top value above p_top and the bottom value between p_bot and the surface psurf [ncol][nt] (None: the surface
    is p_bot, nothing below is held); a column whose pressures are not finite and strictly increasing is NaN, and
    with method="log" so is one with a pressure <= 0 (method="linear" takes any finite increasing pressures).
    f, p: [ncol][nlev][nt]; everything in fp64."""
    f = np.asarray(f, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    pt = np.asarray(plev_pa, dtype=np.float64)
    ncol, nlev, nt = f.shape
    surf = p[:, -1, :] if psurf is None else np.asarray(psurf, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = np.log(p) if method == "log" else p
        xt = np.log(pt) if method == "log" else pt
        good = np.all(np.isfinite(p), axis=1) & np.isfinite(surf) & np.all(np.diff(p, axis=1) > 0, axis=1)   # [ncol][nt]
        if method == "log":
            good &= np.all(p > 0, axis=1)
        above = pt[None, :, None] < p[:, :1, :]
        below = pt[None, :, None] > p[:, -1:, :]
        held = below & (pt[None, :, None] <= surf[:, None, :])
    out = np.full((ncol, pt.size, nt), np.nan)
    for i in range(ncol):
        for t in range(nt):
            if good[i, t]:
                out[i, :, t] = np.interp(xt, x[i, :, t], f[i, :, t])
    out[above | below] = np.nan
    if edge == "hold":
        out = np.where(above, f[:, :1, :], out)
        out = np.where(held, f[:, -1:, :], out)
    out[np.broadcast_to(~good[:, None, :], out.shape)] = np.nan
    return out


def hybrid_levels(nlev=72):
    """Hybrid coefficients of a model with its top at 0.1 hPa: pure pressure above eta = 0.2, terrain following below."""
    eta = np.exp(np.linspace(np.log(1e-4), np.log(0.9976), nlev))
    b = np.maximum((eta - 0.2) / 0.8, 0.0) ** 1.3
    return eta - b, b


def surface_pressure(lat, lon, nt):
    """The surface of test_missing_host.surface_mask, in Pa: 1e5 +- 1500, a southern polar cap at 6.5e4, a plateau at
    6e4.  [ncol][nt]."""
    lat = np.asarray(lat)[:, None]
    lon = np.asarray(lon)[:, None]
    t = np.arange(nt)[None, :]
    ps = 1000.0 + 15.0 * np.sin(np.deg2rad(lon) + 0.7 * t) * np.cos(np.deg2rad(lat))
    ps = np.where(lat < -70.0, 650.0, ps)
    plateau = (np.abs(lat - 33.0) < 8.0) & (np.abs(lon - 88.0) < 15.0)
    return np.where(plateau, 600.0, ps) * 100.0


def hybrid_pressure(hyam, hybm, ps, p0=1e5):
    return hyam[None, :, None] * p0 + hybm[None, :, None] * ps[:, None, :]


def model_fields(lat, lon, nlev, nt, n=4, seed=5, dtype=np.float64):
    """n smooth fields on nlev model levels (the analytic fields and tracers at the levels' nominal pressures)."""
    from pytemdiags_amd import synth
    nominal = np.exp(np.linspace(np.log(0.1), np.log(997.6), nlev))
    fs = list(synth.analytic_fields(lat, lon, nominal, nt, seed=seed))
    fs += [synth.analytic_tracer(lat, lon, nominal, nt, which=i % 2, seed=100 + i) for i in range(max(0, n - 4))]
    return [np.ascontiguousarray(x.astype(dtype)) for x in fs[:n]]


def atmosphere_on_model_levels(lat, lon, p, nt, seed=3, dtype=np.float64):
    """ua, va, ta, wap of one atmosphere sampled on model levels: the analytic fields evaluated at each point's own
    pressure p [ncol][nlev][nt] in Pa, so that what the interpolation returns is that atmosphere on pressure levels.
    (model_fields places the profiles at nominal pressures whatever the surface pressure is.  That suits the kernel
    tests, which only need smooth numbers, but over the plateau and the polar cap it squeezes the whole profile above
    600 hPa; the zonal mean d(theta)/dp the TEM formulas divide by then comes close to zero on the lowest levels, and
    the oracle itself moves by 5e-11 (vtem, field-normalised) when its inputs move by 1e-15, against 2e-13 for the
    pressure-level fields the pipeline's 1e-10 parity tolerance was set on: test_frontend_fixture_is_well_conditioned.)"""
    from pytemdiags_amd import synth
    return [np.ascontiguousarray(x) for x in synth.analytic_fields(lat, lon, p / 100.0, nt, seed=seed, dtype=dtype)]


def frontend_case(nt=2, nlev=72, dtype=np.float64):
    """The ne8 fixture with an atmosphere that is consistent with its surface pressure."""
    lat, lon, hyam, hybm, ps = case_ne8(nt=nt, nlev=nlev)
    f = atmosphere_on_model_levels(lat, lon, hybrid_pressure(hyam, hybm, ps), nt, dtype=dtype)
    return lat, lon, hyam, hybm, ps, f


def inside_everywhere(p, plev_pa):
    """Target levels that lie inside every column."""
    return (plev_pa >= p[:, 0, :].max()) & (plev_pa <= p[:, -1, :].min())


def assert_no_edge_ties(p, plev_pa):
    """A condition on the inputs: no target within 1e-9 (in ln p) of a column's first or last level, so the NaN
    pattern has no rounding ties and a GPU test may demand identical patterns with nothing excluded.  (The surface
    needs no such margin: a target is compared with ps itself, which both sides hold exactly.)"""
    lt = np.log(plev_pa)[None, :, None]
    for edge in (p[:, :1, :], p[:, -1:, :]):
        assert np.min(np.abs(lt - np.log(edge))) > 1e-9


def case_ne8(nt=3, nlev=72):
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(8)
    hyam, hybm = hybrid_levels(nlev)
    ps = surface_pressure(lat, lon, nt)
    return lat, lon, hyam, hybm, ps


# ---- fixtures of test_gpu_vertical_edges.py ------------------------------------------------------------------------
VERT_THREADS = 256


def slab_shape(nf, nlev, nt, nplev, tsz, psz):
    """Host mirror of vert_slab_shape (launch_shapes.hpp), which test_slab_shape_mirrors_the_library holds it to: the
    LDS budget, the 256 / nt cap on cw, seg = max(4, ceil(brackets / most)).  psz is 0 in hybrid mode.  None: the slab
    map cannot take the shape.  Only the tests use it, to assert that their shapes hit the regimes they name."""
    if nt > VERT_THREADS // 4:
        return None
    in_stride, out_stride = (nlev * nt) | 1, (nplev * nt) | 1
    percol = nf * (in_stride + out_stride) * tsz + in_stride * psz
    budget = 48 * 1024 - VERT_THREADS * 4 - (2 * nf + 1) * 16
    cw = min(budget // percol, VERT_THREADS // nt)
    if cw < 1:
        return None
    most = VERT_THREADS // (cw * nt)
    seg = max(4, (nlev - 1 + most - 1) // most)
    return dict(cw=cw, seg=seg, nseg=(nlev - 1 + seg - 1) // seg, in_stride=in_stride, out_stride=out_stride)


# (nf, nlev, nt, nplev, field dtype, pressure mode, pressure dtype, ncol % cw, what vert_slab_shape makes of it)
F64, F32 = np.float64, np.float32
SWEEP = [
    (1, 2, 1, 1, F32, "hybrid", F64, 5, dict(cw=256, nseg=1)),       # 256 / nt cap; a float4 spans two columns
    (1, 2, 1, 1, F64, "hybrid", F64, 5, dict(cw=256, nseg=1)),
    (1, 3, 1, 2, F32, "field", F32, 5, dict(cw=256, nseg=1)),
    (4, 5, 1, 3, F64, "hybrid", F64, 50, dict(cw=187, nseg=1)),       # cw limited by LDS, colsz 5 and 3 odd
    (4, 6, 3, 5, F64, "field", F64, 11, dict(cw=38, seg=4, nseg=2)),
    (8, 9, 5, 7, F32, "hybrid", F32, 7, dict(cw=18, nseg=2)),
    (4, 13, 1, 5, F64, "hybrid", F64, 20, dict(cw=83, nseg=3)),
    (5, 17, 3, 6, F32, "field", F64, 9, dict(cw=26, seg=6, nseg=3)),
    (4, 26, 2, 11, F64, "hybrid", F32, 6, dict(cw=19, seg=5, nseg=5)),
    (3, 33, 7, 9, F64, "field", F32, 2, dict(cw=6, seg=6, nseg=6)),
    (4, 21, 4, 9, F64, "field", F64, 4, dict(cw=10, nseg=5)),
    (8, 128, 3, 37, F64, "field", F64, 0, dict(cw=1, nseg=32)),       # one column per workgroup: no residue to choose
    (1, 1000, 1, 37, F64, "hybrid", F64, 2, dict(cw=5, seg=20, nseg=50)),   # A > 300
    (8, 1000, 1, 37, F64, "hybrid", F64, 0, None),                    # one column does not fit: lanes along time
    (2, 10, 64, 4, F64, "hybrid", F64, 1, dict(cw=3, nseg=1)),        # wide rows, slab only when forced
    (1, 6, 64, 3, F32, "hybrid", F64, 2, dict(cw=4)),
    (2, 9, 15, 5, F64, "hybrid", F64, 5, dict()),                     # the switch points of the default map
    (2, 9, 16, 5, F64, "field", F64, 5, dict()),
    (2, 9, 31, 5, F32, "hybrid", F32, 3, dict()),
    (2, 9, 32, 5, F32, "field", F32, 3, dict()),
]


def sweep_id(case):
    nf, nlev, nt, nplev, dt, pmode, pdt, res, _ = case
    return "nf%d-nlev%d-nt%d-nplev%d-%s-%s_%s-res%d" % (nf, nlev, nt, nplev, np.dtype(dt).name, pmode,
                                                       np.dtype(pdt).name, res)


def sweep_ncol(case):
    """At least three workgroups in either map (cw columns a workgroup in the slab map, 256 (column, time) pairs along
    time), and the stated number of columns in the last slab workgroup."""
    nf, nlev, nt, nplev, dt, pmode, pdt, res, _ = case
    sh = slab_shape(nf, nlev, nt, nplev, np.dtype(dt).itemsize, 0 if pmode == "hybrid" else np.dtype(pdt).itemsize)
    cw = sh["cw"] if sh else 1
    n = max(3 * cw + 1, -(-(2 * VERT_THREADS + 1) // nt))
    while n % cw != res:
        n += 1
    return n


def rough_case(ncol, nlev, nt, nf, pmode, dtype=np.float64, p_dtype=np.float64, seed=0):
    """Random columns for the edge tests.  Levels: log-spaced between 10 Pa and 9.9e4 Pa, each moved by at most 0.3 of
    the spacing (by at most 0.3 in ln p, which matters for 2 or 3 levels only, and at 128 levels by 0.22 of the spacing,
    which keeps the amplification below 300).  field: per (column, time), as the
    pressure array P.  hybrid: the levels are moved once and split into hyam + hybm (pure pressure above eta = 0.2), ps
    is uniform in [8e4, 1.04e5] Pa.  Fields are rough in the vertical: white noise per level plus a column offset, so a
    value from a neighbouring bracket or column is wrong at order 1.
    Returns dict(f, p (fp64, what the kernel sees), P or ps in p_dtype, hyam, hybm, psurf)."""
    rng = np.random.default_rng(1000 + seed)
    base = np.linspace(np.log(10.0), np.log(9.9e4), nlev)
    d = base[1] - base[0]
    move = 0.3 * min(d, 1.0)
    if d > 0.05:      # where the spacing allows it (up to 128 levels), keep ln p / d ln p <= ln(1.3e5) / 0.0406 = 290
        move = min(move, 0.5 * (d - 0.0406))
    out = dict(hyam=None, hybm=None, ps=None, P=None, psurf=None)
    if pmode == "field":
        P = np.exp(base[None, :, None] + move * rng.uniform(-1.0, 1.0, (ncol, nlev, nt))).astype(p_dtype)
        out.update(P=P, p=P.astype(np.float64))
    else:
        x = base.copy()
        x[1:-1] += move * rng.uniform(-1.0, 1.0, nlev - 2)
        eta = np.exp(x) / 1e5
        b = np.maximum((eta - 0.2) / 0.8, 0.0) ** 1.3
        ps = rng.uniform(8e4, 1.04e5, (ncol, nt)).astype(p_dtype)
        out.update(hyam=eta - b, hybm=b, ps=ps, psurf=ps.astype(np.float64))
        out["p"] = hybrid_pressure(out["hyam"], out["hybm"], out["psurf"])
    assert np.all(np.diff(out["p"], axis=1) > 0)
    out["f"] = [np.ascontiguousarray((rng.standard_normal((ncol, nlev, nt)) + 3.0 * rng.standard_normal((ncol, 1, 1)))
                                     .astype(dtype)) for _ in range(nf)]
    return out


def rough_targets(nplev, seed=0):
    """nplev targets in hPa between 5 Pa and 1.05e5 Pa.  The first six are placed: 970 hPa (in a bracket, held or below
    the surface, by column), 0.07 (above every top), 30 and 30.03 (one bracket), 1000 and 1040; the rest are random."""
    placed = [970.0, 0.07, 30.0, 30.03, 1000.0, 1040.0]
    rng = np.random.default_rng(2000 + seed)
    rest = np.exp(rng.uniform(np.log(0.05), np.log(1050.0), max(0, nplev - len(placed))))
    t = np.sort(np.concatenate([placed[:nplev], rest]))
    assert t.size == nplev and np.all(np.diff(t) > 0)
    return t


def target_classes(p, pt, psurf=None):
    """Number of (column, time, target) triples per class: above the top, in a bracket, between the bottom level and
    the surface, below the surface (field mode: below the bottom level), and in a bracket that holds two or more."""
    ptb = pt[None, :, None]
    above = ptb < p[:, :1, :]
    under = ptb > p[:, -1:, :]
    surf = p[:, -1, :] if psurf is None else psurf
    held = under & (ptb <= surf[:, None, :])
    k = np.stack([np.searchsorted(p[i, :, t], pt, side="left") for i in range(p.shape[0]) for t in range(p.shape[2])])
    inside = ~(above | under).transpose(0, 2, 1).reshape(k.shape)
    shared = inside[:, 1:] & inside[:, :-1] & (k[:, 1:] == k[:, :-1])
    return dict(above=int(above.sum()), bracket=int(inside.sum()), held=int(held.sum()), below=int((under & ~held).sum()),
                shared=int(shared.sum()))


def classes_expected(nplev, pmode):
    """What the shape allows: the placed targets come in the order of rough_targets."""
    want = {"bracket", "below"}
    if pmode == "hybrid":
        want.add("held")
    if nplev >= 2:
        want.add("above")
    if nplev >= 4:
        want.add("shared")
    return want


def amplification(p, method):
    """A = max x_k / (x_k - x_{k-1}), x = ln p or p: what the fp64 bound of check() is derived from (A < 300)."""
    x = np.log(p) if method == "log" else p
    return float(np.max(x[:, 1:, :] / np.diff(x, axis=1)))


# (nlev, nt, pressure mode, nf, dtype of ps): nf is the one at which vert_slab_shape cuts 26 levels into segments of 5
# brackets (seams at 5, 10, 15, 20) and 13 levels into segments of 4 (seams at 4, 8) in that mode
TIE_CASES = [(26, 2, "field", 3, np.float64), (13, 1, "field", 4, np.float64), (26, 2, "hybrid", 4, np.float64),
             (13, 1, "hybrid", 4, np.float64), (26, 2, "hybrid", 4, np.float32)]


def tie_ncol(nlev, nt, pmode, nf):
    return 3 * slab_shape(nf, nlev, nt, {26: 11, 13: 9}[nlev], 8, 0 if pmode == "hybrid" else 8)["cw"] + 7


def tie_case(nlev, nt, ncol, nf=4, ps_dtype=np.float64, seed=0):
    """Exact ties.  Every pressure is a small dyadic number, so that the products below are exact:
    level k has the nominal pressure (H_k / 64) hPa, H_k an integer; a target is plev_hpa * 100.0 with plev_hpa = H / 64.
    p0 = 102400 Pa.  Upper levels (the first 16 of 26, 9 of 13): hybm = 0, hyam = H_k / 65536, so p = hyam p0 = H_k 100 / 64
    in every column.  Lower levels: hybm = n_k / 256, hyam = (4 H_k - 995 n_k) / 2^18, so p = H_k 100 / 64 exactly
    where ps = 99500 Pa (a third of the columns; 995 hPa is a target too) and varies with ps elsewhere.
    Targets: above the top, level 0, every `seams` level, two other levels, one inside the bracket before a seam, the
    bottom level, the surface of the tied columns.  Returns the case and the number of tied triples it intends."""
    rng = np.random.default_rng(3000 + seed)
    nup = {26: 16, 13: 9}[nlev]
    seams = {26: (5, 10, 15, 20), 13: (4, 8)}[nlev]
    others = {26: (3, 12), 13: (2, 6)}[nlev]
    H = np.round(np.exp(np.linspace(np.log(10.0), np.log(9.9e4), nlev)) / 100.0 * 64.0).astype(np.int64)
    assert np.all(np.diff(H) > 0) and H[-1] * 100 // 64 < 99500
    g = np.where(np.arange(nlev) < nup, 0.0, np.linspace(0.0, 0.99, nlev - nup + 1)[np.maximum(np.arange(nlev) - nup + 1, 0)])
    n = np.round(256.0 * g * (H * 100.0 / 64.0) / 99500.0).astype(np.int64)
    assert np.all(n[:nup] == 0) and np.all(n[nup:] > 0) and np.all(4 * H - 995 * n >= 0)
    hybm = n / 256.0
    hyam = (4 * H - 995 * n) / 2.0 ** 18
    p0 = 102400.0
    ps = rng.uniform(8e4, 1.04e5, (ncol, nt))
    star = np.arange(ncol) % 3 == 1
    ps[star, :] = 99500.0
    ps = ps.astype(ps_dtype)
    ps64 = ps.astype(np.float64)
    p = hybrid_pressure(hyam, hybm, ps64, p0)
    assert np.all(np.diff(p, axis=1) > 0)
    mid = (H[seams[1] - 1] + H[seams[1]]) // 2
    tied_levels = sorted({0, nlev - 1, *seams, *others})
    hs = sorted([4, mid, 995 * 64] + [int(H[k]) for k in tied_levels])
    plev_hpa = np.array(hs, dtype=np.float64) / 64.0
    pt = plev_hpa * 100.0
    assert np.all(np.diff(pt) > 0) and np.array_equal(pt.astype(np.float32).astype(np.float64), pt)
    assert np.array_equal(p[star], np.broadcast_to((H * 100.0 / 64.0)[None, :, None], p[star].shape))
    upper = sum(1 for k in tied_levels if k < nup)
    lower = len(tied_levels) - upper
    intended = upper * ncol * nt + lower * int(star.sum()) * nt
    f = [np.ascontiguousarray(rng.standard_normal((ncol, nlev, nt)) + 3.0 * rng.standard_normal((ncol, 1, 1)))
         for _ in range(nf)]
    return dict(f=f, p=p, ps=ps, psurf=ps64, hyam=hyam, hybm=hybm, p0=p0, plev_hpa=plev_hpa, pt=pt, star=star,
                seams=seams, tied_levels=tied_levels, H=H), intended


# ---- the fixtures are what the GPU tests assume -------------------------------------------------------------------
def test_fixture_has_no_target_on_a_column_edge():
    """The shapes the GPU tests run: no edge ties, a few per cent of the targets below ground, 23 levels inside every
    column, and the amplification ln p / d ln p the fp64 tolerance is derived from."""
    for nlev, nt in ((72, 3), (128, 3), (72, 91), (128, 30)):
        lat, lon, hyam, hybm, ps = case_ne8(nt=nt, nlev=nlev)
        p = hybrid_pressure(hyam, hybm, ps)
        assert np.all(np.diff(p, axis=1) > 0)
        assert_no_edge_ties(p, PLEV37 * 100.0)
        outside = (PLEV37[None, :, None] * 100.0 > p[:, -1:, :]) | (PLEV37[None, :, None] * 100.0 < p[:, :1, :])
        assert 0.01 < outside.mean() < 0.10                       # a few per cent of the targets are below ground
        assert int(inside_everywhere(p, PLEV37 * 100.0).sum()) == 23
        x = np.log(p)
        assert np.max(x[:, 1:, :] / np.diff(x, axis=1)) < 300      # the amplification the fp64 tolerance is derived from


def test_frontend_fixture_is_well_conditioned():
    """A condition on the inputs of the end-to-end test against the oracle, checked on the oracle alone.  Two correct
    interpolations differ by roundings (the kernel and np.interp do not take the same logarithms or blend in the same
    order), about 1e-15 of a value.  The 1e-10 tolerance of the pipeline can only be asked of what comes after if such a
    difference in the fields moves the oracle's own results by far less: at most 1e-12, a hundredth of it.  (The
    pressure-level fields the tolerance was set on move by 2e-13; these move by about as much.)"""
    from conftest import fieldnorm_err
    from oracle import tem_oracle as orc
    lat, lon, hyam, hybm, ps, f = frontend_case()
    p = hybrid_pressure(hyam, hybm, ps)
    levels = PLEV37[inside_everywhere(p, PLEV37 * 100.0)]
    g = [interp_ref(x, p, levels * 100.0, psurf=ps) for x in f]
    rng = np.random.default_rng(0)
    moved = [x * (1.0 + 1e-15 * rng.uniform(-1.0, 1.0, x.shape)) for x in g]
    a = orc.TEMOracle(*g, lat, levels, L=30, mode="factorised")
    b = orc.TEMOracle(*moved, lat, levels, L=30, mode="factorised")
    for n in ("vtem", "omegatem", "wtem", "psitem", "epfy", "epfz", "epdiv", "utendepfd", "utendvtem", "utendwtem"):
        e = fieldnorm_err(getattr(b, n)(), getattr(a, n)())
        print("%s: %.3e" % (n, e))
        assert e <= 1e-12, (n, e)


def test_sweep_shapes_hit_the_regimes_they_name():
    """The geometry sweep of test_gpu_vertical_edges.py: every case has the slab shape its entry claims, at least three
    workgroups in both maps with the stated residue in the last one, ncol * nt small enough for the reference loop,
    targets in every class the shape allows, and the amplification the fp64 bound is derived from (or, for the two
    1000-level cases, the A that scales it)."""
    seen = set()
    for case in SWEEP:
        nf, nlev, nt, nplev, dt, pmode, pdt, res, claim = case
        sh = slab_shape(nf, nlev, nt, nplev, np.dtype(dt).itemsize, 0 if pmode == "hybrid" else np.dtype(pdt).itemsize)
        if claim is None:
            assert sh is None and nt <= 64                      # refused for LDS, not for the row length
        else:
            assert sh is not None and all(sh[k] == v for k, v in claim.items()), (sweep_id(case), sh)
            assert sh["nseg"] * sh["cw"] * nt <= VERT_THREADS
            seen.add((min(sh["nseg"], 4), sh["cw"] == VERT_THREADS // nt, sh["in_stride"] == nlev * nt))
        ncol = sweep_ncol(case)
        cw = sh["cw"] if sh else 1
        assert ncol % cw == res and ncol > 2 * cw and ncol * nt > 2 * VERT_THREADS and ncol * nt <= 20000
        assert cw <= 2 or 0 < res < cw - 1, sweep_id(case)
        c = rough_case(ncol, nlev, nt, 1, pmode, dt, pdt)
        got = target_classes(c["p"], rough_targets(nplev) * 100.0, c["psurf"])
        for name in classes_expected(nplev, pmode):
            assert got[name] > 0, (sweep_id(case), name, got)
        a = max(amplification(c["p"], "log"), amplification(c["p"], "linear"))
        print("%s: cw %s, ncol %d, A = %.0f, classes %s" % (sweep_id(case), cw, ncol, a, got))
        assert (a < 300) == (nlev < 1000), (sweep_id(case), a)
        assert a < 5000
    # one to four and more segments; cw at the 256 / nt cap and below it; odd and even column blocks
    assert {x[0] for x in seen} == {1, 2, 3, 4} and {x[1] for x in seen} == {True, False} and {x[2] for x in seen} == {True, False}
    # a block of columns shorter than one 16-byte vector, and nt on both sides of the default map's switch (128-byte rows)
    assert any(c[1] * c[2] * np.dtype(c[4]).itemsize < 16 for c in SWEEP)
    assert {(c[2] * np.dtype(c[4]).itemsize) for c in SWEEP if not c[8] and c[8] is not None} == {120, 128, 124}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_slab_shape_mirrors_the_library(build, tmp_path_factory):
    """The real vert_slab_shape, run through tests/host/host_tables_main.cpp on every row of SWEEP and TIE_CASES (and
    on rows that are too long for the slab map): slab_shape agrees field for field, the refusals included."""
    from test_host_tables import runner, vert_cases
    cases = np.concatenate([vert_cases(), [[2, 9, 65, 5, 8, 0], [1, 2, 200, 1, 4, 4]]])
    out = runner(build, tmp_path_factory)("vert", cases)["vert"].reshape(-1, 10)
    assert len(cases) == len(SWEEP) + len(TIE_CASES) + 2
    for (nf, nlev, nt, nplev, tsz, psz), o in zip(cases.astype(np.int64).tolist(), out.tolist()):
        ok, cw, nseg, seg, in_stride, out_stride, in_img, out_img, p_img, lds = o
        sh = slab_shape(nf, nlev, nt, nplev, tsz, psz)
        if sh is None:
            assert ok == 0, (nf, nlev, nt, nplev, tsz, psz)
            continue
        assert ok == 1 and dict(cw=cw, seg=seg, nseg=nseg, in_stride=in_stride, out_stride=out_stride) == sh
        r16 = lambda b: (b + 15) // 16 * 16
        assert (in_img, out_img, p_img) == (r16(cw * in_stride * tsz), r16(cw * out_stride * tsz), r16(cw * in_stride * psz))
        assert lds == VERT_THREADS * 4 + p_img + nf * (in_img + out_img) <= 48 * 1024
    assert sum(1 for o in out.tolist() if o[0] == 0) == 3


def test_unaligned_and_count_fixtures_are_well_conditioned():
    for nf, nlev, nt, nplev in ((4, 6, 3, 5), (3, 5, 1, 3), (8, 9, 3, 6), (8, 9, 20, 6), (13, 9, 3, 6), (2, 5, 2, 4)):
        for pmode in ("hybrid", "field"):
            c = rough_case(150, nlev, nt, 1, pmode)
            assert max(amplification(c["p"], "log"), amplification(c["p"], "linear")) < 300


def test_tie_fixture_holds_the_ties_it_intends():
    """Ties counted straight from the arrays equal the number the construction intends; a third of the surfaces are
    tied as well; the slab shapes cut the columns at the seams named; the amplification stays below 300."""
    for nlev, nt, pmode, nf, psd in TIE_CASES:
        sh = slab_shape(nf, nlev, nt, {26: 11, 13: 9}[nlev], 8, 0 if pmode == "hybrid" else 8)
        ncol = tie_ncol(nlev, nt, pmode, nf)
        c, intended = tie_case(nlev, nt, ncol, nf, psd)
        assert c["pt"].size == {26: 11, 13: 9}[nlev]
        assert tuple(range(sh["seg"], nlev - 1, sh["seg"])) == c["seams"], (sh, c["seams"])
        ties = c["pt"][None, None, :, None] == c["p"][:, :, None, :]          # [ncol][nlev][nplev][nt]
        assert int(ties.sum()) == intended and intended >= 100, (int(ties.sum()), intended)
        for k in c["tied_levels"]:
            assert ties[c["star"], k].any() and (k >= {26: 16, 13: 9}[nlev] or ties[:, k].any(axis=1).all())
        surf = c["pt"][None, :, None] == c["psurf"][:, None, :]
        assert int(surf.sum()) == int(c["star"].sum()) * nt and c["star"].sum() >= ncol // 3
        assert max(amplification(c["p"], "log"), amplification(c["p"], "linear")) < 300
        got = target_classes(c["p"], c["pt"], c["psurf"])
        assert all(got[k] > 0 for k in ("above", "bracket", "held", "below")), got


def test_reference_non_positive_pressure_is_a_bad_column_in_log_mode_only():
    """Interface-level data has p_0 = 0: ln p does not exist, so method="log" returns NaN for the whole (column, time);
    method="linear" takes it like any finite increasing column.  Neighbouring columns are untouched."""
    c = rough_case(12, 9, 2, 1, "field")
    pt = rough_targets(6) * 100.0
    good = {m: interp_ref(c["f"][0], c["p"], pt, m, "hold") for m in ("log", "linear")}
    q = c["p"].copy()
    q[3, 0, 1] = 0.0
    q[7, 0, :] = -5.0
    out = interp_ref(c["f"][0], q, pt, "log", "hold")
    assert np.all(np.isnan(out[3, :, 1])) and np.all(np.isnan(out[7]))
    keep = np.ones(out.shape, bool)
    keep[3, :, 1] = keep[7] = False
    assert np.array_equal(out[keep], good["log"][keep], equal_nan=True) and np.isfinite(out[keep]).any()
    lin = interp_ref(c["f"][0], q, pt, "linear", "hold")
    assert np.isfinite(lin[3, :, 1]).any() and np.isfinite(lin[7]).any()
    assert np.array_equal(lin[keep], good["linear"][keep], equal_nan=True)
    # hybrid: hyam[0] = hybm[0] = 0 puts p_0 = 0 into every column
    h = rough_case(5, 9, 2, 1, "hybrid")
    h["hyam"][0] = h["hybm"][0] = 0.0
    p = hybrid_pressure(h["hyam"], h["hybm"], h["psurf"])
    assert np.all(np.isnan(interp_ref(h["f"][0], p, pt, "log", "hold", psurf=h["psurf"])))
    assert np.isfinite(interp_ref(h["f"][0], p, pt, "linear", "hold", psurf=h["psurf"])).any()


# ---- self-checks of the reference ---------------------------------------------------------------------------------
def _small(nt=2, ncol=40):
    rng = np.random.default_rng(7)
    hyam, hybm = hybrid_levels(72)
    ps = rng.uniform(5.5e4, 1.03e5, (ncol, nt))
    return hyam, hybm, ps, hybrid_pressure(hyam, hybm, ps)


def test_reference_reproduces_a_field_linear_in_log_p():
    hyam, hybm, ps, p = _small()
    f = 3.0 - 2.5 * np.log(p)
    pt = PLEV37 * 100.0
    out = interp_ref(f, p, pt)
    want = np.broadcast_to((3.0 - 2.5 * np.log(pt))[None, :, None], out.shape)
    fin = np.isfinite(out)
    assert fin.any() and np.max(np.abs(out[fin] - want[fin])) <= 1e-13 * np.max(np.abs(want))
    lin = interp_ref(1.0 + 2e-4 * p, p, pt, method="linear")
    assert np.array_equal(np.isfinite(lin), fin)
    assert np.max(np.abs(lin[fin] - np.broadcast_to((1.0 + 2e-4 * pt)[None, :, None], out.shape)[fin])) <= 1e-13 * 21.0


def test_reference_hold_differs_from_nan_only_outside_the_column():
    hyam, hybm, ps, p = _small()
    rng = np.random.default_rng(1)
    f = rng.standard_normal(p.shape)
    pt = np.concatenate([[5.0], PLEV37 * 100.0])                  # 0.05 hPa: above the model top
    a = interp_ref(f, p, pt, edge="nan")
    h = interp_ref(f, p, pt, edge="hold", psurf=ps)
    inside = (pt[None, :, None] >= p[:, :1, :]) & (pt[None, :, None] <= p[:, -1:, :])
    assert np.array_equal(a[inside], h[inside]) and np.all(np.isfinite(a[inside])) and np.all(np.isnan(a[~inside]))
    assert np.array_equal(h[:, 0, :], f[:, 0, :])                 # held above the top
    between = (pt[None, :, None] > p[:, -1:, :]) & (pt[None, :, None] <= ps[:, None, :])
    below = pt[None, :, None] > ps[:, None, :]
    assert between.any() and below.any()
    assert np.array_equal(h[between], np.broadcast_to(f[:, -1:, :], h.shape)[between]) and np.all(np.isnan(h[below]))
    # field mode: the surface is the bottom level, nothing below it is held
    hf = interp_ref(f, p, pt, edge="hold")
    assert np.all(np.isnan(hf[pt[None, :, None] > p[:, -1:, :]]))


def test_reference_bad_columns_and_nan_values():
    hyam, hybm, ps, p = _small()
    f = np.random.default_rng(2).standard_normal(p.shape)
    pt = PLEV37 * 100.0
    good = interp_ref(f, p, pt)
    q = p.copy()
    q[3, 40, 1] = q[3, 39, 1]                                     # not strictly increasing
    q[5, 10, 0] = np.nan
    out = interp_ref(f, q, pt)
    assert np.all(np.isnan(out[3, :, 1])) and np.all(np.isnan(out[5, :, 0]))
    keep = np.ones(out.shape, bool)
    keep[3, :, 1] = keep[5, :, 0] = False
    assert np.array_equal(out[keep], good[keep], equal_nan=True)
    g = f.copy()
    g[7, 50, 0] = np.nan                                          # reaches the brackets (49, 50) and (50, 51) only
    out = interp_ref(g, p, pt)
    touched = (pt > p[7, 49, 0]) & (pt < p[7, 51, 0])
    assert touched.any() and np.all(np.isnan(out[7, touched, 0]))
    assert np.array_equal(out[7, ~touched, 0], good[7, ~touched, 0], equal_nan=True)


# ---- validation before any device call ----------------------------------------------------------------------------
def test_validation_errors_are_raised_without_a_device():
    from pytemdiags_amd import interp_to_pressure
    hyam, hybm = hybrid_levels(8)
    f = np.zeros((5, 8, 2))
    ps = np.full((5, 2), 1e5)
    ok = dict(ps=ps, hyam=hyam, hybm=hybm)
    with pytest.raises(ValueError, match="exactly one"):
        interp_to_pressure(f, [500.0], hyam=hyam, hybm=hybm)
    with pytest.raises(ValueError, match="exactly one"):
        interp_to_pressure(f, [500.0], p=np.zeros_like(f), **ok)
    with pytest.raises(ValueError, match="hyam"):
        interp_to_pressure(f, [500.0], ps=ps, hyam=hyam)
    with pytest.raises(ValueError, match="method"):
        interp_to_pressure(f, [500.0], method="cubic", **ok)
    with pytest.raises(ValueError, match="edge"):
        interp_to_pressure(f, [500.0], edge="extrapolate", **ok)
    with pytest.raises(ValueError, match="repeated"):
        interp_to_pressure(f, [500.0, 700.0, 700.0], **ok)
    with pytest.raises(ValueError, match="shape"):
        interp_to_pressure([f, np.zeros((5, 7, 2))], [500.0], **ok)
    with pytest.raises(ValueError, match="ps has shape"):
        interp_to_pressure(f, [500.0], ps=np.full((4, 2), 1e5), hyam=hyam, hybm=hybm)
    with pytest.raises(ValueError, match="p has shape"):
        interp_to_pressure(f, [500.0], p=np.zeros((5, 8, 3)))
    with pytest.raises(ValueError, match="levels"):
        interp_to_pressure(f, [500.0], ps=ps, hyam=hyam[:-1], hybm=hybm[:-1])
    # monotone at the largest surface pressure, not at the smallest: one reduction over ps finds it
    a = np.linspace(1e-3, 0.3, 8)
    b = np.array([0, 0, 0, 0, 0.1, 0.35, 0.55, 0.7])
    b[5], a[5] = 0.2, a[4] - 0.047                                # p_5 - p_4 = 0.1 ps - 0.047 p0 < 0 for ps < 4.7e4
    psv = np.full((5, 2), 1e5)
    psv[2, 1] = 3e4
    with pytest.raises(ValueError, match="not strictly increasing"):
        interp_to_pressure(f, [500.0], ps=psv, hyam=a, hybm=b)
    with pytest.raises(ValueError, match="not strictly increasing"):
        interp_to_pressure(f, [500.0], ps=ps, hyam=hyam[::-1], hybm=hybm[::-1])     # bottom first


def test_from_model_levels_validates_before_a_device():
    from pytemdiags_amd import TEMDiagnostics
    hyam, hybm = hybrid_levels(8)
    f = np.zeros((5, 8, 2))
    lat = np.linspace(-80, 80, 5)
    ps = np.full((5, 2), 1e5)
    with pytest.raises(ValueError, match="exactly one"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=[500.0], hyam=hyam, hybm=hybm)
    with pytest.raises(NotImplementedError, match="tracers"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=[500.0], ps=ps, hyam=hyam, hybm=hybm, q=f,
                                         missing="mask")
    with pytest.raises(ValueError, match="missing"):
        TEMDiagnostics.from_model_levels(f, f, f, f, lat, plev=[500.0], ps=ps, hyam=hyam, hybm=hybm, missing="bogus")


# ---- header, bindings, plain-C consumer ---------------------------------------------------------------------------
def test_vert_header_declares_exactly_what_is_bound():
    from pytemdiags_amd import _lib, _vert
    hdr = open(os.path.join(ROOT, "include", "temx_vert.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(temxv_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _vert.SIGNATURES}
    assert not re.findall(r"\b(temx_[a-z0-9_]+)\s*\(", code)      # the first header's ABI is not extended from here
    lib = _vert.load()
    assert lib is _lib.load() and lib.temxv_version() == _vert.VERT_VERSION == 100
    for name, value in (("TEMXV_P_HYBRID", _vert.P_HYBRID), ("TEMXV_P_FIELD", _vert.P_FIELD), ("TEMXV_LOG", _vert.LOG),
                        ("TEMXV_LINEAR", _vert.LINEAR), ("TEMXV_EDGE_NAN", _vert.EDGE_NAN),
                        ("TEMXV_EDGE_HOLD", _vert.EDGE_HOLD), ("TEMXV_NF_MAX", _vert.NF_MAX)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    # every temxv entry point with a body is a function-try-block, like the entry points of temx.h
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    assert re.search(r"^int temxv_interp\([^;{]*\)\s*try \{\s*$", src, re.M)


def test_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _vert
    lib = _vert.load()
    plev = (C.c_double * 2)(5e4, 7e4)
    bad_plev = (C.c_double * 2)(7e4, 5e4)
    hy = (C.c_double * 3)(0.1, 0.2, 0.3)
    src, dst = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(1 << 20)

    def call(nf=1, src=src, dst=dst, dtype=0, plev=plev, pmode=0, hyam=hy, hybm=hy, ps=C.c_void_p(1 << 24), method=0,
             edge=0):
        # device 99 does not exist: a call that got as far as the device would come back TEMX_EHIP, not TEMX_EINVAL
        return lib.temxv_interp(99, nf, src, dst, dtype, 4, 3, 2, 2, plev, pmode, hyam, hybm, 1e5, ps, 0, method, edge,
                                None)
    assert call(nf=0) == -1 and b"nf" in lib.temx_last_error()
    assert call(nf=9) == -1
    assert call(src=None) == -1 and call(dst=None) == -1 and call(plev=None) == -1 and call(ps=None) == -1
    assert call(hyam=None) == -1
    assert call(src=(C.c_void_p * 1)(None)) == -1
    assert call(plev=bad_plev) == -1 and call(plev=(C.c_double * 2)(-1.0, 5e4)) == -1
    assert call(dtype=2) == -1 and call(pmode=2) == -1 and call(method=2) == -1 and call(edge=-1) == -1
    assert call(dst=src) == -1 and b"overlaps" in lib.temx_last_error()
    assert call(dst=(C.c_void_p * 1)(4096 + 64)) == -1            # partial overlap is aliasing too
    assert call() == -2                                           # well-formed: only now is the device touched


def test_vert_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_vert")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_vert.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxv_version=100" in out.stdout and "nf0_rc=-1" in out.stdout
