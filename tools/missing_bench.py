#!/usr/bin/env python3
"""Timing of the missing-value mode (TEMX_OPT_MISSING = 1) against the default and the generic paths, one process.

ne120 x 72 x 30 fp64 by default: synthetic fields (temx_synth_fields) with the points below a synthetic surface
pressure set to NaN (southern polar cap at 650 hPa, a plateau at 600 hPa, +-15 hPa with time elsewhere; the mask of
tests/test_missing_host.py).  Each mode: warm-up, then the median of --reps runs of tem_run timed with HIP events.
Prints one JSON line (and writes it to --out when given).

  python tools/missing_bench.py [--ne 120 --nlev 72 --nt 30 --reps 20 --out profiles/missing_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytemdiags_amd import engine, synth  # noqa: E402


def surface_missing(lat, lon, plev, nt, dev):
    lat = torch.as_tensor(lat, device=dev)[:, None]
    lon = torch.as_tensor(lon, device=dev)[:, None]
    t = torch.arange(nt, device=dev, dtype=torch.float64)[None, :]
    ps = 1000.0 + 15.0 * torch.sin(torch.deg2rad(lon) + 0.7 * t) * torch.cos(torch.deg2rad(lat))
    ps = torch.where(lat < -70.0, torch.full_like(ps, 650.0), ps)
    plateau = ((lat - 33.0).abs() < 8.0) & ((lon - 88.0).abs() < 15.0)
    ps = torch.where(plateau, torch.full_like(ps, 600.0), ps)
    p = torch.as_tensor(plev, device=dev)[None, :, None]
    return p > ps[:, None, :]


def timed(plan, f, out, reps):
    plan.tem_run(*f, out=out)
    plan.tem_run(*f, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plan.tem_run(*f, out=out)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=120)
    ap.add_argument("--nlev", type=int, default=72)
    ap.add_argument("--nt", type=int, default=30)
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-masked", action="store_true", help="one masked configuration (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lat, lon = synth.cubed_sphere_gll(a.ne)
    plev = synth.pressure_levels(a.nlev)
    lat_zm = (np.arange(-90, 91, 1.0)[1:] + np.arange(-90, 91, 1.0)[:-1]) / 2
    f = engine.synth_fields(0, lat, lon, plev, a.nt, dtype=torch.float64)
    miss = surface_missing(lat, lon, plev, a.nt, dev)
    fm = [torch.where(miss, torch.full_like(x, float("nan")), x) for x in f]
    rec = {"grid": "ne%d" % a.ne, "ncol": int(lat.size), "nlev": a.nlev, "nt": a.nt, "L": a.L, "dtype": "float64",
           "missing_fraction": float(miss.double().mean().item()), "reps": a.reps}
    modes = [("masked", dict(), True)]
    if not a.only_masked:
        modes += [("default", dict(), False), ("generic", dict(symmetry=False), False)]
    for name, kw, masked in modes:
        plan = engine.Plan(lat, lat_zm, a.L, device=0, **kw)
        if masked:
            plan.configure(missing="mask")
        plan.set_tem(a.nlev, a.nt, plev * 100)
        out = plan._alloc_results(False)
        med, lo, hi = timed(plan, fm if masked else f, out, a.reps)
        rec[name + "_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        if masked:
            cov = plan.coverage()
            rec["coverage_nan_fraction"] = float((cov < 0.5).double().mean().item())
            rec["results_finite"] = bool(torch.isfinite(out[0][0]).any().item())
        plan.close()
        del out
        torch.cuda.empty_cache()
    if not a.only_masked:
        rec["masked_over_generic"] = round(rec["masked_ms"]["median"] / rec["generic_ms"]["median"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
