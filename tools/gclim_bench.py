#!/usr/bin/env python3
"""Timing of temxg_time_sum_groups (the grouped, weighted time sum of fields in engine layout, include/temx_gclim.h),
one process, a time limit per leg.  (The per-leg limit is an alarm the interpreter answers between calls; a leg stuck
inside a blocking device call is ended only from outside: run the tool under ``timeout -k 10 <seconds>``.)

Legs, 4 fields each: ne120 x 72 x 30 fp64 and fp32 with two contiguous groups of 15 (staged rows), ne30 x 72 x 730 fp64
with 24 contiguous month-like groups and with 4 seasonal groups that lie in pieces (the long-row kernel).  Two
yardsticks, in the same process on the same tensors:
  * ``temxc_time_sum``, unchanged: it reads the same bytes, so the ratio says what grouping costs;
  * the torch composition a user would write: ``torch.matmul(x, Wm)`` with ``Wm[t][g] = w_t [label_t == g]``, after
    ``x.double()`` for fp32 fields.
Reported: median ms of --reps runs after --warm warm-ups (HIP events), bytes read per second, both ratios, and the
worst |kernel - matmul| over the derived bound 2 (n_g + 1) 2^-53 sum |w x|.  ``climatology.GROUP_SUM_KERNEL[dtype]``
follows ``torch_over_kernel_time`` at ne120 x 72 x 30 (tests/test_gclim_host.py holds it to this file's output).

  python tools/gclim_bench.py [--reps 20 --warm 3 --out profiles/gclim_bench_mi355x.json]
"""
import argparse
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytemdiags_amd import _gclim, engine, synth  # noqa: E402

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


def labels_of(groups, nt):
    """(labels, ng) of a leg: "2 contiguous", "24 contiguous" (month-like runs), "4 seasonal" (runs of a quarter of a
    year of 365 / 2 steps that repeat: every group lies in pieces)."""
    n, kind = groups.split()
    n = int(n)
    t = np.arange(nt)
    if kind == "contiguous":
        return ((t * n) // nt).astype(np.int32), n
    per_year = 365.0
    return (np.floor((t % per_year) / per_year * n).astype(np.int32) % n), n


def leg(plan, name, ne, nlev, nt, dtype, groups, reps, warm):
    ncol = synth.ncol_of_ne(ne)
    g = torch.Generator(device=DEV).manual_seed(1)
    fields = [torch.randn((ncol, nlev, nt), generator=g, device=DEV, dtype=dtype) for _ in range(4)]
    labels, ng = labels_of(groups, nt)
    w = np.random.default_rng(2).uniform(0.5, 1.5, nt)
    wm = np.zeros((nt, ng))
    wm[np.arange(nt), labels] = w
    wm_d = torch.as_tensor(wm, device=DEV)
    acc = list(torch.empty((4, ncol, nlev, ng), dtype=torch.float64, device=DEV).unbind(0))
    plain = list(torch.empty((4, ncol, nlev), dtype=torch.float64, device=DEV).unbind(0))
    k = stats_ms(lambda: plan.time_sum_groups(fields, labels, ng, w, acc=acc), reps, warm)
    p = stats_ms(lambda: plan.time_sum(fields, acc=plain), reps, warm)
    t = stats_ms(lambda: [torch.matmul(x.double(), wm_d) for x in fields], reps, warm)
    ref = torch.matmul(fields[0].double(), wm_d)
    scale = torch.matmul(fields[0].double().abs(), wm_d)
    n_g = torch.as_tensor(np.bincount(labels, minlength=ng).astype(np.float64), device=DEV)
    rel = float(((acc[0] - ref).abs() / (2.0 * (n_g + 1.0) * 2.0 ** -53 * scale)).max())
    del ref, scale
    esz = fields[0].element_size()
    nbytes = 4 * ncol * nlev * nt * esz
    present = int(np.unique(labels).size)
    staged = nt < _gclim.switch_nt(esz)
    rec = {"leg": name, "ncol": ncol, "nlev": nlev, "nt": nt, "dtype": str(dtype).replace("torch.", ""), "nf": 4,
           "groups": groups, "ng": ng,
           "kernel": "staged" if staged else "long-row, bound %d" % _gclim.bound(present),
           "bytes_read": nbytes, "bytes_written": 4 * ncol * nlev * ng * 8,
           "kernel_ms": round(k[0], 4), "kernel_ms_min_max": [round(k[1], 4), round(k[2], 4)],
           "time_sum_ms": round(p[0], 4), "time_sum_ms_min_max": [round(p[1], 4), round(p[2], 4)],
           "torch_ms": round(t[0], 4), "torch_ms_min_max": [round(t[1], 4), round(t[2], 4)],
           "kernel_read_TBps": round(nbytes / k[0] / 1e9, 3), "time_sum_read_TBps": round(nbytes / p[0] / 1e9, 3),
           "kernel_over_time_sum_time": round(k[0] / p[0], 3), "torch_over_kernel_time": round(t[0] / k[0], 3),
           "max_delta_over_bound_vs_torch": rel}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--leg-limit", type=int, default=180, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--out", default="profiles/gclim_bench_mi355x.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gclim_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    lat, _ = synth.cubed_sphere_gll(4)[:2]
    plan = engine.Plan(lat, np.arange(-89.5, 90, 1.0), 10, device=0)     # (the sums use the plan's device only)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm,
           "switch_nt": {"float64": _gclim.switch_nt(8), "float32": _gclim.switch_nt(4)}, "bounds": list(_gclim.BOUNDS),
           "time_sum_groups": []}
    shapes = [("ne120x72x30_f64_2", 120, 72, 30, torch.float64, "2 contiguous"),
              ("ne120x72x30_f32_2", 120, 72, 30, torch.float32, "2 contiguous"),
              ("ne30x72x730_f64_24", 30, 72, 730, torch.float64, "24 contiguous"),
              ("ne30x72x730_f64_4s", 30, 72, 730, torch.float64, "4 seasonal")]
    rc = 0
    for n, ne, nl, nt, dt, gr in shapes:
        signal.alarm(a.leg_limit)
        try:
            rec["time_sum_groups"].append(leg(plan, n, ne, nl, nt, dt, gr, a.reps, a.warm))
        except LegTimeout:
            rec.setdefault("errors", []).append({"leg": n, "error": "over the leg limit of %d s" % a.leg_limit})
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
