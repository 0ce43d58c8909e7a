#!/usr/bin/env python3
"""Timing of the latitude-bin form (TEMX_OPT_LAT_BINS) against the generic sweeps it is an alternative to, one process.

ne120 x 72 x 30 fp64 by default, fields generated on the device (temx_synth_fields).  The grid is the cubed sphere with
its latitudes jittered by a seeded +-1e-3 degrees, so that no two columns share a latitude and the plan's own sweeps
are the generic ones (sweep_mode 0).  Legs, all on one plan: the generic form, the binned form at the default number
of bins, at 256 and 1024 bins, and the generic and the default binned form again on fp32 fields.  Each leg: 3 warm-ups,
then median and min-max of --reps runs of tem_run timed with HIP events; then the two sweeps alone through
temx_kernel_timing (5 more runs); the binned legs also carry their parity with the generic leg (ten results and 16
zonal intermediates, field-normalised) and their time as a multiple of the floor of two reads of the fields at the
6.29 TB/s of a float4 copy.  Prints one JSON line and writes it to --out.

  python tools/binned_bench.py [--ne 120 --nlev 72 --nt 30 --reps 20 --out profiles/binned_bench_mi355x.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytemdiags_amd import engine, synth  # noqa: E402

COPY_TBS = 6.29        # measured float4 copy, TB/s
BIN_ROWS = 512         # rows per chunk (csrc/bin_tables.hpp)


def workspace_bytes(lat, bins, J, K, D):
    """What the binned form allocates (csrc/temx.hip, bin_setup and bin_workspace), from the same bin rule."""
    edges = -0.5 * np.pi + np.arange(bins + 1) * (np.pi / bins)
    counts = np.bincount(np.searchsorted(edges[1:-1], lat * (np.pi / 180.0), side="right"), minlength=bins)
    nchunk = int(np.sum(-(-counts // BIN_ROWS)))
    dpad, kp = -(-D // 64) * 64, -(-K // 16) * 16
    ws = {"chunks": nchunk, "chunk_moments": nchunk * 4 * J * dpad * 8, "series": bins * 4 * J * dpad * 8,
          "coefficients": 4 * K * D * 8, "tables": bins * J * kp * 8 + 2 * kp * kp * 8,
          "rows": lat.size * 12 + nchunk * 16 + (bins + 1) * 4}
    ws["total"] = sum(v for k, v in ws.items() if k != "chunks")
    return ws


def leg(plan, f, reps, warm=3):
    out = plan._alloc_results(True)
    for _ in range(warm):
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
    plan.kernel_timing(True)
    for _ in range(5):
        plan.tem_run(*f, out=out)
    assert not plan.status()
    k0, k1 = plan.kernel_timing_read(0)[0], plan.kernel_timing_read(1)[0]
    plan.kernel_timing(False)
    med = float(np.median(ms))
    rec = {"median_ms": round(med, 3), "min_ms": round(float(np.min(ms)), 3), "max_ms": round(float(np.max(ms)), 3),
           "sweep1_ms": round(k0, 3), "sweep2_ms": round(k1, 3), "rest_ms": round(med - k0 - k1, 3),
           "form": plan.sweep_form, "sweep_mode": plan.sweep_mode}
    return rec, out


def parity(out, ref):
    worst = 0.0
    for x, r in zip(out, ref):
        for i in range(x.shape[0]):
            worst = max(worst, float(((x[i] - r[i]).abs().max() / r[i].abs().max()).item()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=120)
    ap.add_argument("--nlev", type=int, default=72)
    ap.add_argument("--nt", type=int, default=30)
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="profiles/binned_bench_mi355x.json")
    a = ap.parse_args()
    lat, lon = synth.cubed_sphere_gll(a.ne)
    lat = np.clip(lat + np.random.default_rng(17).uniform(-1e-3, 1e-3, lat.size), -90.0, 90.0)
    plev = synth.pressure_levels(a.nlev)
    lat_zm = (np.arange(-90, 91, 1.0)[1:] + np.arange(-90, 91, 1.0)[:-1]) / 2
    rec = {"grid": "ne%d, latitudes jittered by +-1e-3 degrees" % a.ne, "ncol": int(lat.size), "nlev": a.nlev, "nt": a.nt,
           "L": a.L, "reps": a.reps, "device": torch.cuda.get_device_name(0), "legs": {}}
    for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
        f = engine.synth_fields(0, lat, lon, plev, a.nt, dtype=dtype)
        floor_ms = 2 * 4 * f[0].numel() * f[0].element_size() / (COPY_TBS * 1e12) * 1e3
        plan = engine.Plan(lat, lat_zm, a.L, device=0, fp32_fields=dtype == torch.float32)
        plan.set_tem(a.nlev, a.nt, plev * 100)
        g, ref = leg(plan, f, a.reps)
        g["floor_ms"] = round(floor_ms, 3)
        rec["legs"]["generic_" + tag] = g
        for bins in ((512, 256, 1024) if dtype == torch.float64 else (512,)):
            plan.configure(lat_bins=bins)
            plan.set_tem(a.nlev, a.nt, plev * 100)
            b, out = leg(plan, f, a.reps)
            b.update(bins=plan.lat_bins, bin_degree=plan.bin_degree, parity_with_generic=float("%.3g" % parity(out, ref)),
                     floor_ms=round(floor_ms, 3), over_floor=round(b["median_ms"] / floor_ms, 3),
                     over_generic=round(b["median_ms"] / g["median_ms"], 3),
                     ranges_overlap=bool(b["max_ms"] >= g["min_ms"]),
                     workspace_bytes=workspace_bytes(lat, plan.lat_bins, plan.bin_degree, a.L + 1, a.nlev * a.nt))
            rec["legs"]["binned%d_%s" % (bins, tag)] = b
            del out
        plan.close()
        del f, ref
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
