#!/usr/bin/env python3
"""Timing of temxw_time_sum_groups_valid (the grouped, weighted sum over the valid times of fields in engine layout,
pytemdiags_amd/include/temx_mgclim.h), one process, a time limit per leg.  (The per-leg limit is an alarm the interpreter
answers between calls; a leg stuck inside a blocking device call is ended only from outside: run the tool under
``timeout -k 10 <seconds>``.)

Legs, 4 fields under a common below-surface mask each: ne120 x 72 x 30 fp64 and fp32 with two contiguous groups of 15
(staged rows), ne30 x 72 x 730 fp64 with 12 contiguous month-like groups (long rows, LDS form) and with 4 seasonal groups
that lie in pieces (long rows, registers), and ne30 x 72 x 121 and x 255 fp64 with two groups, where the rows are still
staged but only 8 and 4 of them fit a workgroup's four images.  Yardsticks, in the same process on the same tensors:
  * ``temxn_time_sum_valid`` on the masked fields and ``temxg_time_sum_groups`` on zero-filled copies, both unchanged:
    they read the same bytes, so the ratios say what grouping costs the masked sum and what the mask costs the grouped one;
  * the torch composition a user would write: ``isfinite``, ``all`` over the fields, ``where``, then three kinds of
    ``matmul`` with the ``[NT][G]`` weight matrix (the sums, the weights, the counts).
Reported: median ms of --reps runs after --warm warm-ups (HIP events) with min and max, bytes read per second, the three
ratios, and the worst |kernel - torch| of the sums over the derived bound 2 (n_g + 1) 2^-53 sum |w x|.

  python tools/mgclim_bench.py [--reps 20 --warm 3 --out profiles/mgclim_bench_mi355x.json]
"""
import argparse
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytemdiags_amd import _mgclim, engine, synth  # noqa: E402

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
    """(labels, ng) of a leg: "2 contiguous", "12 contiguous" (month-like runs), "4 seasonal" (runs of a quarter of a
    year of 365 / 2 steps that repeat: every group lies in pieces)."""
    n, kind = groups.split()
    n = int(n)
    t = np.arange(nt)
    if kind == "contiguous":
        return ((t * n) // nt).astype(np.int32), n
    per_year = 365.0
    return (np.floor((t % per_year) / per_year * n).astype(np.int32) % n), n


def surface_missing(ncol, nlev, nt):
    """A below-surface mask on the device, bool [ncol][nlev][nt]: levels linear from 10 to 1010 hPa under a surface
    pressure of 1000 hPa +- 15 hPa that moves with time, and a patch of columns under a plateau at 600 hPa."""
    c = torch.arange(ncol, device=DEV, dtype=torch.float64)[:, None]
    t = torch.arange(nt, device=DEV, dtype=torch.float64)[None, :]
    ps = 1000.0 + 15.0 * torch.sin(c * (6.283185307179586 / 997.0) + 0.7 * t)
    ps = torch.where((c % 50.0) < 2.0, torch.full_like(ps, 600.0), ps)
    plev = torch.linspace(10.0, 1010.0, nlev, device=DEV, dtype=torch.float64)
    return plev[None, :, None] > ps[:, None, :]


def r4(x):
    return [round(v, 4) for v in x]


def leg(plan, name, ne, nlev, nt, dtype, groups, reps, warm):
    ncol = synth.ncol_of_ne(ne)
    g = torch.Generator(device=DEV).manual_seed(1)
    miss = surface_missing(ncol, nlev, nt)
    fields = []
    for _ in range(4):
        x = torch.randn((ncol, nlev, nt), generator=g, device=DEV, dtype=dtype)
        x[miss] = float("nan")
        fields.append(x)
    missing_share = float(miss.double().mean())
    del miss
    labels, ng = labels_of(groups, nt)
    w = np.random.default_rng(2).uniform(0.5, 1.5, nt)
    wm = np.zeros((nt, ng))
    wm[np.arange(nt), labels] = w
    wm_d = torch.as_tensor(wm, device=DEV)
    ind_d = torch.as_tensor((wm > 0).astype(np.float64), device=DEV)

    def outs(n):
        return list(torch.empty((n, ncol, nlev, ng), dtype=torch.float64, device=DEV).unbind(0))
    acc, (wsum,), (cnt,) = outs(4), outs(1), outs(1)
    k = stats_ms(lambda: plan.time_sum_groups_valid(fields, labels, ng, w, acc=acc, wsum=wsum, cnt=cnt), reps, warm)
    vacc = list(torch.empty((4, ncol, nlev), dtype=torch.float64, device=DEV).unbind(0))
    vcnt = torch.empty((ncol, nlev), dtype=torch.float64, device=DEV)
    v = stats_ms(lambda: plan.time_sum_valid(fields, acc=vacc, cnt=vcnt), reps, warm)
    del vacc, vcnt

    def composition():
        ok = torch.isfinite(fields[0])
        for x in fields[1:]:
            ok &= torch.isfinite(x)
        okd = ok.double()
        zero = torch.zeros((), dtype=fields[0].dtype, device=DEV)
        sums = [torch.matmul(torch.where(ok, x, zero).double(), wm_d) for x in fields]
        return sums, torch.matmul(okd, wm_d), torch.matmul(okd, ind_d)
    t = stats_ms(composition, reps, warm)
    sums, tw, tc = composition()
    scale = torch.matmul(torch.nan_to_num(fields[0], nan=0.0).double().abs(), wm_d)
    n_g = torch.as_tensor(np.bincount(labels, minlength=ng).astype(np.float64), device=DEV)
    bound = 2.0 * (n_g + 1.0) * 2.0 ** -53 * scale
    rel = float(((acc[0] - sums[0]).abs() / torch.clamp(bound, min=1e-300)).max())
    counts_equal = bool(torch.equal(cnt, tc))
    del sums, tw, tc, scale, bound
    torch.cuda.empty_cache()
    filled = [torch.nan_to_num(x, nan=0.0) for x in fields]
    gacc = outs(4)
    gs = stats_ms(lambda: plan.time_sum_groups(filled, labels, ng, w, acc=gacc), reps, warm)
    del filled, gacc
    esz = fields[0].element_size()
    nbytes = 4 * ncol * nlev * nt * esz
    present = int(np.unique(labels).size)
    sh = _mgclim.shape(ncol * nlev, nt, esz, 4, present)
    form = "staged, %d rows per workgroup" % sh["rpb"] if sh["staged"] else ("long-row, registers, bound %d" % sh["bound"] if sh["bound"] < 64 else
                                          "long-row, LDS, %d pass%s, %d waves per workgroup" % (sh["npass"], "es" if sh["npass"] > 1 else "", sh["rpw"]))
    rec = {"leg": name, "ncol": ncol, "nlev": nlev, "nt": nt, "dtype": str(dtype).replace("torch.", ""), "nf": 4,
           "groups": groups, "ng": ng, "kernel": form, "missing_share": round(missing_share, 4),
           "bytes_read": nbytes, "bytes_written": 6 * ncol * nlev * ng * 8,
           "kernel_ms": round(k[0], 4), "kernel_ms_min_max": r4(k[1:]),
           "time_sum_valid_ms": round(v[0], 4), "time_sum_valid_ms_min_max": r4(v[1:]),
           "time_sum_groups_ms": round(gs[0], 4), "time_sum_groups_ms_min_max": r4(gs[1:]),
           "torch_ms": round(t[0], 4), "torch_ms_min_max": r4(t[1:]),
           "kernel_read_TBps": round(nbytes / k[0] / 1e9, 3),
           "kernel_over_valid_time": round(k[0] / v[0], 3), "kernel_over_valid_time_min_max": r4([k[1] / v[2], k[2] / v[1]]),
           "kernel_over_grouped_time": round(k[0] / gs[0], 3), "kernel_over_grouped_time_min_max": r4([k[1] / gs[2], k[2] / gs[1]]),
           "torch_over_kernel_time": round(t[0] / k[0], 3), "torch_over_kernel_time_min_max": r4([t[1] / k[2], t[2] / k[1]]),
           "max_delta_over_bound_vs_torch": rel, "counts_equal_torch": counts_equal}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--leg-limit", type=int, default=180, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--out", default="profiles/mgclim_bench_mi355x.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mgclim_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    lat, _ = synth.cubed_sphere_gll(4)[:2]
    plan = engine.Plan(lat, np.arange(-89.5, 90, 1.0), 10, device=0)     # (the sums use the plan's device only)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm,
           "switch_nt": {"float64": _mgclim.switch_nt(8), "float32": _mgclim.switch_nt(4)}, "bounds": list(_mgclim.BOUNDS),
           "lds_batch": {str(n): _mgclim.batch(n) for n in (1, 4, 8)}, "time_sum_groups_valid": []}
    shapes = [("ne120x72x30_f64_2", 120, 72, 30, torch.float64, "2 contiguous"),
              ("ne120x72x30_f32_2", 120, 72, 30, torch.float32, "2 contiguous"),
              ("ne30x72x730_f64_12", 30, 72, 730, torch.float64, "12 contiguous"),
              ("ne30x72x730_f64_4s", 30, 72, 730, torch.float64, "4 seasonal"),
              # staged rows beyond the nt at which 16 rows of four fp64 images fit (64): 8 and 4 rows per workgroup
              ("ne30x72x121_f64_2", 30, 72, 121, torch.float64, "2 contiguous"),
              ("ne30x72x255_f64_2", 30, 72, 255, torch.float64, "2 contiguous")]
    rc = 0
    for n, ne, nl, nt, dt, gr in shapes:
        signal.alarm(a.leg_limit)
        try:
            rec["time_sum_groups_valid"].append(leg(plan, n, ne, nl, nt, dt, gr, a.reps, a.warm))
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
