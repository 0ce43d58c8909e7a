#!/usr/bin/env python3
"""Timing of the masked tracer run (include/temx_mtracer.h) against the masked TEM run and the unmasked two-pass tracer
run, one process.

ne120 x 72 x 30 fp64 by default: synthetic fields and one tracer (temx_synth_fields; the tracer is a smooth positive
function of the temperature field) with the points below a synthetic surface pressure set to NaN in all five arrays --
the mask of tools/missing_bench.py, the tracer missing where the fields are.  Per call: --warmup runs, then the median
of --reps runs timed with HIP events; a run that takes longer than --step-limit seconds ends the process.  The split
into projection (+ its reduction) and eddy sweep comes from the library's own event pairs (temx_kernel_timing).
Prints one JSON line (and writes it to --out when given).  With --kernel-trace DIR the record also gets the per-kernel
averages of a rocprofv3 --kernel-trace csv found under DIR (a run of this tool with --only-masked), and --table-out
gets that table as text.

  python tools/masked_tracer_bench.py [--ne 120 --nlev 72 --nt 30 --reps 20 --out profiles/masked_tracer_bench_mi355x.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from missing_bench import surface_missing  # noqa: E402
from pytemdiags_amd import engine, synth  # noqa: E402


def timed(call, reps, warmup, limit):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        call()
        b.record()
        b.synchronize()
        if time.perf_counter() - t0 > limit:
            raise SystemExit("a step took %.1f s, over the limit of %.1f s" % (time.perf_counter() - t0, limit))
        ms.append(a.elapsed_time(b))
    return {"median": round(float(np.median(ms)), 3), "min": round(float(np.min(ms)), 3), "max": round(float(np.max(ms)), 3)}


def split(plan):
    """(projection + reduction, eddy sweep) averages in ms of the launches since kernel_timing(True)."""
    return {"projection_ms": round(plan.kernel_timing_read(0)[0], 3), "sweep_ms": round(plan.kernel_timing_read(1)[0], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=120)
    ap.add_argument("--nlev", type=int, default=72)
    ap.add_argument("--nt", type=int, default=30)
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-limit", type=float, default=20.0, help="seconds one timed run may take")
    ap.add_argument("--only-masked", action="store_true", help="the masked runs alone (for a kernel trace)")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 --kernel-trace csv of an --only-masked run")
    ap.add_argument("--table-out", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lat, lon = synth.cubed_sphere_gll(a.ne)
    plev = synth.pressure_levels(a.nlev)
    lat_zm = (np.arange(-90, 91, 1.0)[1:] + np.arange(-90, 91, 1.0)[:-1]) / 2
    f = list(engine.synth_fields(0, lat, lon, plev, a.nt, dtype=torch.float64))
    q = 1e-6 * (1.0 + 0.5 * torch.tanh((f[2] - 250.0) / 30.0))
    rec = {"grid": "ne%d" % a.ne, "ncol": int(lat.size), "nlev": a.nlev, "nt": a.nt, "L": a.L, "dtype": "float64",
           "reps": a.reps, "warmup": a.warmup}
    if not a.only_masked:
        plan = engine.Plan(lat, lat_zm, a.L, device=0, symmetry=False)
        plan.set_tem(a.nlev, a.nt, plev * 100)
        out = plan._alloc_results(False)
        plan.tem_run(*f, out=out)
        rec["form_unmasked"] = plan.sweep_form
        rec["tracer_run_unmasked_two_pass_ms"] = timed(lambda: plan.tracer_run(q, f[1], f[3]), a.reps, a.warmup, a.step_limit)
        plan.close()
        del out
        torch.cuda.empty_cache()
    miss = surface_missing(lat, lon, plev, a.nt, dev)
    rec["missing_fraction"] = float(miss.double().mean().item())
    for x in f + [q]:                       # in place: nothing of field size is held twice
        x.masked_fill_(miss, float("nan"))
    del miss
    plan = engine.Plan(lat, lat_zm, a.L, device=0)
    plan.configure(missing="mask")
    plan.set_tem(a.nlev, a.nt, plev * 100)
    out = plan._alloc_results(False)
    plan.kernel_timing(True)
    rec["masked_tem_run_ms"] = timed(lambda: plan.tem_run(*f, out=out), a.reps, a.warmup, a.step_limit)
    rec["masked_tem_run_split"] = split(plan)
    plan.kernel_timing(True)
    rec["masked_tracer_run_ms"] = timed(lambda: plan.tracer_run_masked(q, f[1], f[3]), a.reps, a.warmup, a.step_limit)
    rec["masked_tracer_run_split"] = split(plan)
    plan.kernel_timing(False)
    tres, _, tcov = plan.tracer_run_masked(q, f[1], f[3])
    rec["tracer_coverage_nan_fraction"] = float((tcov < 0.5).double().mean().item())
    rec["tracer_coverage_equals_tem_coverage"] = float((tcov.reshape(plan.M, -1) - plan.coverage()).abs().max().item())
    rec["results_finite"] = bool(torch.isfinite(tres[0]).any().item())
    rec["tracer_over_tem_run"] = round(rec["masked_tracer_run_ms"]["median"] / rec["masked_tem_run_ms"]["median"], 3)
    rec["projection_over_tem_projection"] = round(rec["masked_tracer_run_split"]["projection_ms"] /
                                                  rec["masked_tem_run_split"]["projection_ms"], 3)
    plan.close()
    if a.kernel_trace:
        from kernel_table import table
        rows = table(a.kernel_trace)
        tot = sum(r[0] for r in rows)
        lines = ["%-84s %20s %6s %10s %10s %6s" % ("kernel", "grid", "calls", "avg us", "min us", "%")]
        for t, n, avg, mn, name, grid in rows[:16]:
            lines.append("%-84s %20s %6d %10.1f %10.1f %6.1f" % (name[:84], grid, n, avg, mn, 100 * t / tot))
        rec["kernels_avg_us"] = {name.split("(")[0][:96] + " [" + grid + "]": round(avg, 1) for t, n, avg, mn, name, grid in rows[:16]}
        if a.table_out:
            with open(a.table_out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
