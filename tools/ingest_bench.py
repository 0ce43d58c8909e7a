#!/usr/bin/env python3
"""Timing of temxi_records_to_pressure (time-major model-level records -> pressure levels in engine layout,
include/temx_ingest.h) against the chain it fuses, one process, a time limit per leg.  (The per-leg limit is an alarm
the interpreter answers between calls: it ends a leg that is slow, and nothing more is started after it.  A leg stuck
inside a blocking device call is ended only from outside: run the tool under ``timeout -k 10 <seconds>``.)

Legs, 4 fields on 72 hybrid levels with ps in fp64: ne120 x 72 -> 37 x 30 in fp64 and fp32, ne120 x 72 -> 72 x 16 in
fp64, ne30 x 72 -> 37 x 92 in fp64.  Per leg, in this session:
  * fused   ``vertical.records_to_pressure_device(..., path="fused")``,
  * chain   ``path="chain"``: temxl_to_engine, the transpose of the ps window, temxv_interp,
  * copy    a torch device copy that moves the bytes the fused call has to move (sources and ps read, outputs
            written): the ceiling,
each the median of --reps runs after --warm warm-ups, HIP events around the call; outputs are allocated outside the
timed region for both paths (the chain's intermediate is part of the chain).  Reported: the three times,
chain_over_fused_time, the fused call's fraction of the copy rate, and whether fused and chain gave the same bits.
``vertical.FUSED_RECORDS`` is set from the file this writes and from nothing else.

  python tools/ingest_bench.py [--reps 20 --warm 3 --out profiles/ingest_bench_mi355x.json]
"""
import argparse
import json
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytemdiags_amd import synth, vertical  # noqa: E402

DEV = torch.device("cuda", 0)
PLEV37 = np.array([1, 2, 3, 5, 7, 10, 20, 30, 50, 70, 100, 125, 150, 175, 200, 225, 250, 300, 350, 400, 450, 500, 550,
                   600, 650, 700, 750, 775, 800, 825, 850, 875, 900, 925, 950, 975, 1000], dtype=np.float64)


class LegTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise LegTimeout()


def hybrid_levels(nlev):
    """Top at 0.1 hPa, pure pressure above eta = 0.2, terrain following below (the coefficients of the tests)."""
    eta = np.exp(np.linspace(np.log(1e-4), np.log(0.9976), nlev))
    b = np.maximum((eta - 0.2) / 0.8, 0.0) ** 1.3
    return eta - b, b


def median_ms(fn, reps, warm):
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


def leg(name, ne, nlev, nplev, nt, dtype, reps, warm, nf=4):
    ncol = synth.ncol_of_ne(ne)
    hyam, hybm = hybrid_levels(nlev)
    plev_pa = (PLEV37 if nplev == 37 else np.exp(np.linspace(np.log(1.0), np.log(1000.0), nplev))) * 100.0
    g = torch.Generator(device=DEV).manual_seed(1)
    srcs = [torch.randn((nt, nlev, ncol), generator=g, device=DEV, dtype=dtype) for _ in range(nf)]
    ps = 6e4 + 4.4e4 * torch.rand((nt, ncol), generator=g, device=DEV, dtype=torch.float64)
    kw = dict(hyam=hyam, hybm=hybm, method="log", edge="nan")
    out_f = list(torch.empty((nf, ncol, nplev, nt), dtype=dtype, device=DEV).unbind(0))
    out_c = list(torch.empty((nf, ncol, nplev, nt), dtype=dtype, device=DEV).unbind(0))
    t_f = median_ms(lambda: vertical.records_to_pressure_device(srcs, ps, plev_pa, out=out_f, path="fused", **kw), reps, warm)
    t_c = median_ms(lambda: vertical.records_to_pressure_device(srcs, ps, plev_pa, out=out_c, path="chain", **kw), reps, warm)
    torch.cuda.synchronize()
    same = all(bool(torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))
                    and torch.equal(torch.isnan(a), torch.isnan(b))) for a, b in zip(out_f, out_c))
    nan_frac = float(torch.isnan(out_f[0]).double().mean())
    esz = srcs[0].element_size()
    nbytes = nf * ncol * nt * (nlev + nplev) * esz + ncol * nt * 8
    del out_c
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)
    b = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)
    t_p = median_ms(lambda: b.copy_(a), reps, warm)
    chain_bytes = nbytes + 2 * nf * ncol * nt * nlev * esz + 2 * ncol * nt * 8
    rec = {"leg": name, "ncol": ncol, "nlev": nlev, "nplev": nplev, "nt": nt, "nf": nf,
           "dtype": str(dtype).replace("torch.", ""), "ps_dtype": "float64",
           "fused_bytes": nbytes, "chain_bytes": chain_bytes,
           "fused_ms": round(t_f[0], 4), "fused_ms_min_max": [round(t_f[1], 4), round(t_f[2], 4)],
           "chain_ms": round(t_c[0], 4), "chain_ms_min_max": [round(t_c[1], 4), round(t_c[2], 4)],
           "copy_ms": round(t_p[0], 4), "copy_TBps": round(nbytes / t_p[0] / 1e9, 3),
           "fused_TBps": round(nbytes / t_f[0] / 1e9, 3),
           "chain_over_fused_time": round(t_c[0] / t_f[0], 3),
           "fused_fraction_of_copy_rate": round(t_p[0] / t_f[0], 3),
           "equal_to_chain": bool(same), "nan_fraction": round(nan_frac, 4)}
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--leg-limit", type=int, default=120, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--out", default="profiles/ingest_bench_mi355x.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ingest_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm, "legs": []}
    f64, f32 = torch.float64, torch.float32
    legs = [("ne120x72to37x30_f64", 120, 72, 37, 30, f64), ("ne120x72to37x30_f32", 120, 72, 37, 30, f32),
            ("ne120x72to72x16_f64", 120, 72, 72, 16, f64), ("ne30x72to37x92_f64", 30, 72, 37, 92, f64)]
    rc = 0
    for name, ne, nlev, nplev, nt, dt in legs:
        signal.alarm(a.leg_limit)
        try:
            rec["legs"] += leg(name, ne, nlev, nplev, nt, dt, a.reps, a.warm)
        except LegTimeout:
            rec["legs"].append({"leg": name, "error": "over the leg limit of %d s" % a.leg_limit})
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
