#!/usr/bin/env python3
"""The algebra of the single sweep in plain fp64 numpy, in the regimes of tests/test_gpu_regimes.py:
sharp zonal-mean structure (synth.jet_fields: Gaussian jets and a tanh front of e-folding width w degrees) with eddies
scaled by eps.  For every case of that test -- the same grid, L, nlev, nt, fields and seed -- the eddy-product sums
from the product linearisation (fields shifted by the reference first) are compared with the direct sums
Y^T (a' b'), both taken through the oracle's epilogue: the worst field-normalised difference over the ten TEM
results and the three flux means is the FLOOR of the algebra in exact-order fp64.  The GPU sums in another order
and in MFMA blocks; the test holds it to 4 x this floor where the floor is above 2.5e-11, to 1e-10 elsewhere.

The reference is what the engine fits: degree < 16, on the engine's own subsample -- every S-th class-group of the
row table in table order, S = groups // 32 (class_tables.hpp, build_classes and class_subsample: the subsample of class-groups for the reference
fit"); class_table() restates that order.  `--subsample random` takes a random 1/16 of the columns instead and
`--subsample all` the whole grid, to see what the choice of the sample costs.  The header line of each grid says how
the engine's subsample covers the latitudes (the largest gap in |sin lat| between sampled classes).

    python tools/proto/single_sweep_regimes.py            # every case of the test: a few minutes on a CPU
    python tools/proto/single_sweep_regimes.py ne12       # one grid
"""
import argparse
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import tem_oracle as orc          # noqa: E402
from pytemdiags_amd import synth              # noqa: E402

MB = 4                                        # members of a class per batch (CLS_MB)
WIDTHS, EPS = (8.0, 4.0, 2.0), (1.0, 0.1, 0.01)
# name -> (grid, L, nlev, nt): the cases of tests/test_gpu_regimes.py, part B
GRIDS = {
    "ne12": (lambda: synth.cubed_sphere_gll(12), 50, 16, 4),            # D = 64
    "ne12-ragged": (lambda: synth.cubed_sphere_gll(12), 50, 13, 5),     # D = 65
    "latlon1440": (lambda: synth.latlon_grid(32, 1440), 20, 16, 4),     # long class sides; D = 64
}
RAGGED_CASES = ((4.0, 0.1),)                   # the (width, eps) run on the ragged shape
FIELD_SEED = 1


def class_table(lat, tol=1e-11):
    """The latitude classes of build_classes (class_tables.hpp) for an fp64 plan, in table order: a list of (rows north,
    rows south); consecutive runs of 4 are the class-groups."""
    lat = np.asarray(lat, dtype=np.float64)
    order = np.argsort(np.abs(lat), kind="stable")
    a = np.abs(lat)[order]
    cls = []
    i = 0
    while i < a.size:
        j = i + int(np.searchsorted(a[i:], a[i] + tol, side="right"))
        rows = order[i:j]
        south = lat[rows] < -tol
        cls.append((np.sort(rows[~south]), np.sort(rows[south])))
        i = j
    nb = lambda m: (len(m) + MB - 1) // MB                                   # noqa: E731
    # outsized classes (more than 4 x the batches of the most frequent shape) are cut to that shape
    hist = Counter((len(n), len(s)) for n, s in cls)
    best = max(hist.values())
    typ = min(k for k, v in hist.items() if v == best)
    cap_n, cap_s = max(typ[0], MB), max(typ[1], MB)
    typ_b = max(1, -(-typ[0] // MB) - (-typ[1] // MB))
    out = []
    for n, s in cls:
        if nb(n) + nb(s) <= 4 * typ_b:
            out.append((n, s))
            continue
        parts = max(-(-len(n) // cap_n), -(-len(s) // cap_s))
        for k in range(parts):
            dn, ds = n[k * cap_n:(k + 1) * cap_n], s[k * cap_s:(k + 1) * cap_s]
            if len(dn) or len(ds):
                out.append((dn, ds))
    cls = out
    cls.sort(key=lambda c: (-nb(c[0]), -nb(c[1]), int(c[0][0]) if len(c[0]) else int(c[1][0])))     # (stable)
    # the class-groups of each (batches north, batches south) stratum spread evenly among the others
    ngr = (len(cls) + 3) // 4
    shape = []
    for g in range(ngr):
        grp = cls[4 * g:4 * g + 4]
        shape.append((max(nb(c[0]) for c in grp), max(nb(c[1]) for c in grp)))
    count, seen, key = Counter(shape), Counter(), []
    for g in range(ngr):
        k = (seen[shape[g]] + 0.5) / count[shape[g]]
        seen[shape[g]] += 1
        if g + 1 == ngr and len(cls) % 4:
            k = 2.0
        key.append((k, g))
    key.sort(key=lambda kg: kg[0])                                                                   # (stable)
    return [c for _, g in key for c in cls[4 * g:4 * g + 4]]


def engine_subsample(lat, keep=32):
    """Columns of the engine's reference subsample: every S-th class-group in table order."""
    cls = class_table(lat)
    groups = (len(cls) + 3) // 4
    S = max(1, min(256, groups // keep))
    rows = [np.concatenate(c) for g in range(0, groups, S) for c in cls[4 * g:4 * g + 4]]
    return np.sort(np.concatenate(rows)), S, groups


def spread(lat, idx):
    """Largest gap in |sin lat| between neighbouring sampled latitudes (1 / number of samples if evenly spread)."""
    x = np.unique(np.round(np.abs(np.sin(np.deg2rad(lat[idx]))), 12))
    return float(np.max(np.diff(np.concatenate([[0.0], x, [1.0]])))), x.size


class Model:
    def __init__(self, lat, L):
        self.lat, self.L, self.K = lat, L, L + 1
        K = self.K
        self.Yx = orc.ylm0_matrix_recurrence(lat, 2 * L)
        self.Y = self.Yx[:, :K]
        self.Q, self.R = np.linalg.qr(self.Y)
        xg, wg = np.polynomial.legendre.leggauss(2 * L + 2)
        Yg = orc.ylm0_matrix_recurrence(np.rad2deg(np.arcsin(xg)), 2 * L)
        self.g = np.einsum("q,ql,qm,qk->lmk", 2 * np.pi * wg, Yg[:, :K], Yg[:, :K], Yg)
        self.T = np.einsum("mnk,lk->lmn", self.g, self.Y.T @ self.Yx)
        self.lat_zm = orc.zm_latitudes(1, False)
        self.Yp = orc.ylm0_matrix_recurrence(self.lat_zm, L)

    def coef(self, A):
        return np.linalg.solve(self.R, self.Q.T @ A)

    def direct(self, a, b):
        ap, bp = a - self.Y @ self.coef(a), b - self.Y @ self.coef(b)
        return self.Y.T @ (ap * bp)

    def linearised(self, a, b, ra, rb):
        a, b = a - ra, b - rb
        A, B = self.Yx.T @ a, self.Yx.T @ b
        P = self.Y.T @ (a * b)
        al, be = self.coef(a), self.coef(b)
        Ma = np.einsum("lmk,kd->lmd", self.g, A)
        Mb = np.einsum("lmk,kd->lmd", self.g, B)
        t1 = np.einsum("lmd,md->ld", Ma, be)
        t2 = np.einsum("lmd,md->ld", Mb, al)
        t3 = np.einsum("lmn,md,nd->ld", self.T, al, be)
        return P - t1 - t2 + t3

    def floor(self, f, plev, idx, kr=16):
        """Worst field-normalised difference, linearised against direct, over the ten results and three fluxes."""
        N = self.lat.size
        nlev, nt = f[0].shape[1:]
        th = f[2] * ((orc.P0 / (plev * 100.0)) ** orc.k)[None, :, None]
        F4 = [np.asarray(x, dtype=np.float64).reshape(N, -1) for x in (f[0], f[1], th, f[3])]
        kr = min(kr, self.K)
        q_, r_ = np.linalg.qr(self.Y[idx][:, :kr])
        ref = [self.Y[:, :kr] @ np.linalg.solve(r_, q_.T @ x[idx]) for x in F4]
        shape = (self.lat_zm.size, nlev, nt)
        zmean = lambda x: (self.Yp @ self.coef(x)).reshape(shape)                                   # noqa: E731
        solve = lambda B3: np.linalg.solve(self.R, np.linalg.solve(self.R.T, B3))                   # noqa: E731
        base = {"ub": zmean(F4[0]), "vb": zmean(F4[1]), "thetab": zmean(F4[2]), "wapb": zmean(F4[3])}
        pairs = ((0, 1, "upvpb"), (0, 3, "upwappb"), (1, 2, "vptpb"))
        names = ("vtem", "omegatem", "wtem", "psitem", "epfy", "epfz", "epdiv", "utendepfd", "utendvtem", "utendwtem")
        out = {}
        for form in ("direct", "lin"):
            z = dict(base)
            for ia, ib, key in pairs:
                Fm = self.direct(F4[ia], F4[ib]) if form == "direct" else self.linearised(F4[ia], F4[ib], ref[ia], ref[ib])
                z[key] = (self.Yp @ solve(Fm)).reshape(shape)
            o = orc.TEMOracle.from_zonal_means(z, plev)
            out[form] = {n: np.asarray(getattr(o, n)(), float) for n in names}
            out[form].update({k: z[k] for _, _, k in pairs})
        errs = {n: float(np.max(np.abs(out["lin"][n] - out["direct"][n])) / np.max(np.abs(out["direct"][n]))) for n in out["direct"]}
        worst = max(errs, key=errs.get)
        return errs[worst], worst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("grids", nargs="*", default=list(GRIDS))
    ap.add_argument("--subsample", choices=("engine", "random", "all"), default="engine")
    ap.add_argument("--keep", type=int, default=32, help="class-groups kept by the engine's rule (TEMX_OPT_OS_SUBSAMPLE)")
    ap.add_argument("--suite-fields", action="store_true", help="also synth.analytic_fields as the rest of the suite uses them")
    args = ap.parse_args()
    for name in args.grids:
        make, L, nlev, nt = GRIDS[name]
        lat, lon = make()
        plev = synth.pressure_levels(nlev)
        idx, S, groups = engine_subsample(lat, args.keep)
        gap, nsamp = spread(lat, idx)
        print("# %s: %d columns, L = %d, D = %d x %d; %d class-groups, every %d-th kept: %d columns at %d latitudes, "
              "largest gap in |sin lat| %.3f" % (name, lat.size, L, nlev, nt, groups, S, idx.size, nsamp, gap), flush=True)
        if args.subsample == "random":
            idx = np.sort(np.random.default_rng(5).choice(lat.size, lat.size // 16, replace=False))
        elif args.subsample == "all":
            idx = np.arange(lat.size)
        m = Model(lat, L)
        if args.suite_fields:
            e, w = m.floor(synth.analytic_fields(lat, lon, plev, nt, seed=3), plev, idx)
            print("%-12s analytic_fields        floor %.1e (%s)" % (name, e, w), flush=True)
        cases = RAGGED_CASES if name.endswith("ragged") else [(w, e) for w in WIDTHS for e in EPS]
        for width, eps in cases:
            f = synth.jet_fields(lat, lon, plev, nt, width=width, eps=eps, seed=FIELD_SEED)
            e, w = m.floor(f, plev, idx)
            print("%-12s width %g eps %-5g floor %.1e (%s)" % (name, width, eps, e, w), flush=True)


if __name__ == "__main__":
    main()
