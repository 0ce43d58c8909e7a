#!/usr/bin/env python3
"""Timing of temxn_time_sum_valid (the sum over the valid times of fields with missing values, include/temx_nclim.h)
and of the constructor with and without ``min_time_coverage=``, one process, a time limit per leg.  (The per-leg limit
is an alarm the interpreter answers between calls; a leg stuck inside a blocking device call is ended only from
outside: run the tool under ``timeout -k 10 <seconds>``.)

Time-sum legs, 4 fields with a below-surface mask in the manner of ``tests/test_missing_host.surface_mask`` (a southern
polar cap at 650 hPa, a plateau at 600 hPa, +-15 hPa of variation with time elsewhere): ne120 x 72 x 30 fp64 and fp32
(staged rows) and ne30 x 72 x 730 fp64 (the long-row kernel).  Per leg, median ms of --reps runs after --warm warm-ups
(HIP events) of
  * ``valid``   ``Plan.time_sum_valid(common=True)`` on the masked fields;
  * ``plain``   ``Plan.time_sum`` (temxc_time_sum, unchanged) on NaN-free copies of the same fields: the yardstick,
                because the bytes read are the same;
  * ``torch``   the composition a user would write: an ``isfinite`` per field, the stacked ``all``, ``where``, a sum
                per field, and the count.
and the ratios ``valid_over_plain_time`` and ``torch_over_valid_time``.  No figure is a pass/fail gate.

Constructor leg: ``TEMDiagnostics(missing="mask")`` on device-resident ne120 x 72 x 30 fp64 masked fields with and
without ``climatology=True, min_time_coverage=0.5``, wall time, interleaved.

  python tools/nclim_bench.py [--reps 20 --warm 3 --out profiles/nclim_bench_mi355x.json]
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

from pytemdiags_amd import _nclim, engine, synth  # noqa: E402

DEV = torch.device("cuda", 0)


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


def levels(nlev):
    """The levels of tests/test_gpu_missing.masked_fields: dense near the surface, hPa."""
    return np.sort(synth.pressure_levels(nlev) * 0.5 + 500.0 * np.linspace(0, 1, nlev) ** 2)


def surface_mask_device(lat, lon, plev, nt):
    """tests/test_missing_host.surface_mask on the device: True = missing, [ncol][nlev][nt]."""
    la = torch.as_tensor(lat, device=DEV, dtype=torch.float64)[:, None]
    lo = torch.as_tensor(lon, device=DEV, dtype=torch.float64)[:, None]
    t = torch.arange(nt, device=DEV, dtype=torch.float64)[None, :]
    ps = 1000.0 + 15.0 * torch.sin(torch.deg2rad(lo) + 0.7 * t) * torch.cos(torch.deg2rad(la))
    ps = torch.where(la < -70.0, torch.full_like(ps, 650.0), ps)
    plateau = ((la - 33.0).abs() < 8.0) & ((lo - 88.0).abs() < 15.0)
    ps = torch.where(plateau, torch.full_like(ps, 600.0), ps)
    return torch.as_tensor(plev, device=DEV, dtype=torch.float64)[None, :, None] > ps[:, None, :]


def torch_composition(fields):
    """What a user would write without the kernel: -> (sums, count)."""
    fin = [torch.isfinite(x) for x in fields]
    valid = torch.stack(fin).all(dim=0)
    sums = [torch.sum(torch.where(valid, x, torch.zeros((), dtype=x.dtype, device=x.device)), -1, dtype=torch.float64)
            for x in fields]
    return sums, valid.sum(-1, dtype=torch.float64)


def time_sum_leg(plan, name, ne, nlev, nt, dtype, reps, warm):
    lat, lon = synth.cubed_sphere_gll(ne)[:2]
    ncol = int(lat.size)
    miss = surface_mask_device(lat, lon, levels(nlev), nt)
    g = torch.Generator(device=DEV).manual_seed(1)
    clean = [torch.randn((ncol, nlev, nt), generator=g, device=DEV, dtype=dtype) for _ in range(4)]
    nan = torch.full((), float("nan"), dtype=dtype, device=DEV)
    fields = [torch.where(miss, nan, x) for x in clean]
    frac = float(miss.sum(dtype=torch.float64) / miss.numel())
    del miss
    acc = list(torch.empty((4, ncol, nlev), dtype=torch.float64, device=DEV).unbind(0))
    cnt = torch.empty((ncol, nlev), dtype=torch.float64, device=DEV)
    pacc = list(torch.empty((4, ncol, nlev), dtype=torch.float64, device=DEV).unbind(0))
    # alternated, so that a drift of the machine reaches all three alike
    v = stats_ms(lambda: plan.time_sum_valid(fields, acc=acc, cnt=cnt, common=True), reps, warm)
    p = stats_ms(lambda: plan.time_sum(clean, acc=pacc), reps, warm)
    v2 = stats_ms(lambda: plan.time_sum_valid(fields, acc=acc, cnt=cnt, common=True), reps, warm)
    p2 = stats_ms(lambda: plan.time_sum(clean, acc=pacc), reps, warm)
    t = stats_ms(lambda: torch_composition(fields), max(3, reps // 4), 1)
    sums, count = torch_composition(fields)
    scale = torch.sum(torch.where(torch.isfinite(fields[0]), fields[0], torch.zeros_like(fields[0])).abs().to(torch.float64), -1)
    rel = float(((acc[0] - sums[0]).abs() / (2.0 * nt * 2.0 ** -53 * scale).clamp_min(1e-300)).max())
    esz = fields[0].element_size()
    nbytes = 4 * ncol * nlev * nt * esz
    vm, pm = min(v[0], v2[0]), min(p[0], p2[0])
    rec = {"leg": name, "ncol": ncol, "nlev": nlev, "nt": nt, "dtype": str(dtype).replace("torch.", ""), "nf": 4,
           "kernel": "staged" if nt < _nclim.switch_nt(esz, 4, True) else "long-row", "missing_fraction": round(frac, 5),
           "bytes_read": nbytes, "valid_ms": round(vm, 4), "valid_ms_runs": [round(v[0], 4), round(v2[0], 4)],
           "valid_ms_min_max": [round(min(v[1], v2[1]), 4), round(max(v[2], v2[2]), 4)],
           "plain_ms": round(pm, 4), "plain_ms_runs": [round(p[0], 4), round(p2[0], 4)],
           "plain_ms_min_max": [round(min(p[1], p2[1]), 4), round(max(p[2], p2[2]), 4)],
           "torch_ms": round(t[0], 4), "torch_ms_min_max": [round(t[1], 4), round(t[2], 4)],
           "valid_TBps": round(nbytes / vm / 1e9, 3), "plain_TBps": round(nbytes / pm / 1e9, 3),
           "valid_over_plain_time": round(vm / pm, 3), "torch_over_valid_time": round(t[0] / vm, 3),
           "counts_equal_torch": bool(torch.equal(cnt, count)), "max_delta_over_bound_vs_torch": rel}
    print(json.dumps(rec), flush=True)
    return rec


def constructor_leg(reps):
    from pytemdiags_amd import TEMDiagnostics
    ne, nlev, nt = 120, 72, 30
    lat, lon = synth.cubed_sphere_gll(ne)[:2]
    plev = levels(nlev)
    fields = engine.synth_fields(0, lat, lon, plev, nt)
    miss = surface_mask_device(lat, lon, plev, nt)
    nan = torch.full((), float("nan"), dtype=fields[0].dtype, device=DEV)
    fields = [torch.where(miss, nan, x) for x in fields]
    del miss
    kw = dict(plev=plev, debug_level=0, missing="mask")
    new = dict(climatology=True, min_time_coverage=0.5)
    TEMDiagnostics(*fields, lat, **kw, **new)                        # warm-up: plan tables, allocator
    torch.cuda.synchronize()
    times = {False: [], True: []}
    for _ in range(reps):
        for on in (False, True):
            t0 = time.perf_counter()
            tem = TEMDiagnostics(*fields, lat, **kw, **(new if on else {}))
            torch.cuda.synchronize()
            times[on].append(time.perf_counter() - t0)
            del tem
    rec = {"leg": "constructor", "ncol": int(lat.size), "nlev": nlev, "nt": nt, "dtype": "float64", "reps": reps,
           "masked_s": round(float(np.median(times[False])), 4),
           "masked_s_min_max": [round(min(times[False]), 4), round(max(times[False]), 4)],
           "masked_climatology_s": round(float(np.median(times[True])), 4),
           "masked_climatology_s_min_max": [round(min(times[True]), 4), round(max(times[True]), 4)]}
    rec["masked_climatology_over_masked"] = round(rec["masked_climatology_s"] / rec["masked_s"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--constructor-reps", type=int, default=3)
    ap.add_argument("--skip-constructor", action="store_true")
    ap.add_argument("--leg-limit", type=int, default=180, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--out", default="profiles/nclim_bench_mi355x.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nclim_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    lat, _ = synth.cubed_sphere_gll(4)[:2]
    plan = engine.Plan(lat, np.arange(-89.5, 90, 1.0), 10, device=0)     # (the time sums use the plan's device only)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm,
           "switch_nt_common_4": {"float64": _nclim.switch_nt(8, 4, True), "float32": _nclim.switch_nt(4, 4, True)},
           "time_sum_valid": [], "constructor": None}
    shapes = [("ne120x72x30_f64", 120, 72, 30, torch.float64), ("ne120x72x30_f32", 120, 72, 30, torch.float32),
              ("ne30x72x730_f64", 30, 72, 730, torch.float64)]
    legs = [(n, (lambda n=n, ne=ne, nl=nl, nt=nt, dt=dt: rec["time_sum_valid"].append(
        time_sum_leg(plan, n, ne, nl, nt, dt, a.reps, a.warm)))) for n, ne, nl, nt, dt in shapes]
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
