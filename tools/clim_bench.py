#!/usr/bin/env python3
"""Timing of temxc_time_sum (the time sum of fields in engine layout, include/temx_clim.h) and of the constructor with
and without ``climatology=True``, one process, a time limit per leg.  (The per-leg limit is an alarm the interpreter
answers between calls; a leg stuck inside a blocking device call is ended only from outside: run the tool under
``timeout -k 10 <seconds>``.)

Time-sum legs, 4 fields: ne120 x 72 x 30 fp64 and fp32, ne30 x 72 x 92 fp64 (staged rows) and ne30 x 72 x 730 fp64 (the
long-row kernel), each against what it replaces, ``torch.sum(x, -1, dtype=torch.float64)`` on the same tensors.
Reported: median ms of --reps runs after --warm warm-ups (HIP events), bytes read per second, and that rate as a fraction
of two float4-copy rates: the 6.29 TB/s that tools/relayout_bench.py and tools/ingest_bench.py divide by
(``fraction_of_float4_copy``, comparable with their figures) and the rate of ``dst.copy_(src)`` on 4 GiB of fp32
measured in this process, bytes read + written per second (``fraction_of_measured_copy``); and the ratio to torch.  ``climatology.TIME_SUM_KERNEL[dtype]`` follows the ratio at ne120 x 72 x 30
(tests/test_clim_host.py holds it to this file's output).

Constructor leg: ``TEMDiagnostics`` on device-resident ne120 x 72 x 30 fp64 fields with and without
``climatology=True``, wall time, interleaved.

  python tools/clim_bench.py [--reps 20 --warm 3 --out profiles/clim_bench_mi355x.json]
"""
import argparse
import json
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytemdiags_amd import _clim, engine, synth  # noqa: E402

DEV = torch.device("cuda", 0)
COPY_TBPS = 6.29        # float4 copy on this chip: the denominator of tools/relayout_bench.py


class LegTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise LegTimeout()


def stats_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def float4_copy_TBps(reps, warm):
    src = torch.empty(1 << 30, dtype=torch.float32, device=DEV).normal_()
    dst = torch.empty_like(src)
    med, _, _ = stats_ms(lambda: dst.copy_(src), reps, warm)
    return 2 * src.numel() * 4 / med / 1e9


def time_sum_leg(plan, name, ne, nlev, nt, dtype, reps, warm, copy_tbps):
    ncol = synth.ncol_of_ne(ne)
    g = torch.Generator(device=DEV).manual_seed(1)
    fields = [torch.randn((ncol, nlev, nt), generator=g, device=DEV, dtype=dtype) for _ in range(4)]
    acc = list(torch.empty((4, ncol, nlev), dtype=torch.float64, device=DEV).unbind(0))
    k = stats_ms(lambda: plan.time_sum(fields, acc=acc), reps, warm)
    t = stats_ms(lambda: [torch.sum(x, -1, dtype=torch.float64) for x in fields], reps, warm)
    ref = torch.sum(fields[0], -1, dtype=torch.float64)
    scale = torch.sum(fields[0].abs().to(torch.float64), -1)
    rel = float(((acc[0] - ref).abs() / (2.0 * nt * 2.0 ** -53 * scale)).max())
    nbytes = 4 * ncol * nlev * nt * fields[0].element_size()
    rec = {"leg": name, "ncol": ncol, "nlev": nlev, "nt": nt, "dtype": str(dtype).replace("torch.", ""), "nf": 4,
           "kernel": "staged" if nt < _clim.switch_nt(fields[0].element_size()) else "long-row",
           "bytes_read": nbytes, "kernel_ms": round(k[0], 4), "kernel_ms_min_max": [round(k[1], 4), round(k[2], 4)],
           "torch_ms": round(t[0], 4), "torch_ms_min_max": [round(t[1], 4), round(t[2], 4)],
           "kernel_TBps": round(nbytes / k[0] / 1e9, 3), "fraction_of_float4_copy": round(nbytes / k[0] / 1e9 / COPY_TBPS, 3),
           "fraction_of_measured_copy": round(nbytes / k[0] / 1e9 / copy_tbps, 3),
           "torch_over_kernel_time": round(t[0] / k[0], 3), "max_delta_over_bound_vs_torch": rel}
    print(json.dumps(rec), flush=True)
    return rec


def constructor_leg(reps):
    from pytemdiags_amd import TEMDiagnostics
    ne, nlev, nt = 120, 72, 30
    lat, lon = synth.cubed_sphere_gll(ne)[:2]
    plev = synth.pressure_levels(nlev)
    fields = engine.synth_fields(0, lat, lon, plev, nt)
    kw = dict(plev=plev, debug_level=0)
    TEMDiagnostics(*fields, lat, climatology=True, **kw)            # warm-up: plan tables, allocator
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            t0 = time.perf_counter()
            tem = TEMDiagnostics(*fields, lat, climatology=on, **kw)
            torch.cuda.synchronize()
            times[on].append(time.perf_counter() - t0)
            path = tem.climatology.time_sum_path if on else None
            del tem
    rec = {"leg": "constructor", "ncol": int(lat.size), "nlev": nlev, "nt": nt, "dtype": "float64", "reps": reps,
           "plain_s": round(float(np.median(times[False])), 4), "plain_s_min_max": [round(min(times[False]), 4), round(max(times[False]), 4)],
           "climatology_s": round(float(np.median(times[True])), 4),
           "climatology_s_min_max": [round(min(times[True]), 4), round(max(times[True]), 4)],
           "time_sum_path": path}
    rec["climatology_over_plain"] = round(rec["climatology_s"] / rec["plain_s"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--constructor-reps", type=int, default=3)
    ap.add_argument("--skip-constructor", action="store_true")
    ap.add_argument("--leg-limit", type=int, default=180, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--out", default="profiles/clim_bench_mi355x.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "clim_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    lat, _ = synth.cubed_sphere_gll(4)[:2]
    plan = engine.Plan(lat, np.arange(-89.5, 90, 1.0), 10, device=0)     # (time_sum uses the plan's device only)
    copy_tbps = float4_copy_TBps(a.reps, a.warm)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm,
           "float4_copy_TBps": COPY_TBPS, "float4_copy_TBps_measured": round(copy_tbps, 3), "switch_nt": {"float64": _clim.switch_nt(8), "float32": _clim.switch_nt(4)},
           "time_sum": [], "constructor": None}
    print(json.dumps({"float4_copy_TBps_measured": rec["float4_copy_TBps_measured"]}), flush=True)
    shapes = [("ne120x72x30_f64", 120, 72, 30, torch.float64), ("ne120x72x30_f32", 120, 72, 30, torch.float32),
              ("ne30x72x92_f64", 30, 72, 92, torch.float64), ("ne30x72x730_f64", 30, 72, 730, torch.float64)]
    legs = [(n, (lambda n=n, ne=ne, nl=nl, nt=nt, dt=dt: rec["time_sum"].append(
        time_sum_leg(plan, n, ne, nl, nt, dt, a.reps, a.warm, copy_tbps)))) for n, ne, nl, nt, dt in shapes]
    if not a.skip_constructor:
        legs.append(("constructor", lambda: rec.__setitem__("constructor", constructor_leg(a.constructor_reps))))
    rc = 0
    for name, fn in legs:
        signal.alarm(a.leg_limit)
        try:
            fn()
        except LegTimeout:
            rec.setdefault("errors", []).append({"leg": name, "error": "over the leg limit of %d s" % a.leg_limit})
            rc = 3
        finally:
            signal.alarm(0)
        if rc:
            break                                                     # nothing more is started after a leg ran over
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    sys.exit(rc)


if __name__ == "__main__":
    main()
