#!/usr/bin/env python3
"""Timing of temxl_to_engine (time-major records -> engine layout, include/temx_layout.h) and of the blocked
constructor, one process, a time limit per leg.  (The per-leg limit is an alarm the interpreter answers between
calls: it ends a leg that is slow, and nothing more is started after it.  A leg stuck inside a blocking device call is
ended only from outside: run the tool under ``timeout -k 10 <seconds>``.)

Kernel legs, 4 fields, at ne120 x 72 x 30 fp64 and fp32 and at ne30 x 72 x 92 fp64, each in this session:
  * temxl_to_engine, against
  * the torch copy it replaces, ``permute(2, 1, 0)`` ... ``.contiguous()``, field by field as the front end did;
both plain, with the level flip (TEMXL_FLIP_LEV against ``torch.flip``) and, for fp32 sources, widening to fp64
(``.to(float64)``).  Reported: median ms (HIP events), bytes read + written per second, the fraction of the 6.29 TB/s
this chip reaches on a float4 copy, and the ratio to the torch copy.

Blocked leg: ``TEMDiagnostics(..., time_block=)`` on a host-resident time-major ne30 x 72 x NT fp32 record (four
fields; --nt 730 is the year of BASELINE configs[2]), upload, re-layout and TEM time per block separately so the
overlap shows, against the path of a whole run without the re-layout (host-side permute + contiguous, pageable upload)
on the prefix --parent-nt of the record.

  python tools/relayout_bench.py [--reps 7 --nt 730 --time-block 32 --out profiles/relayout_bench_mi355x.json]
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

from pytemdiags_amd import layout, synth  # noqa: E402

DEV = torch.device("cuda", 0)
COPY_TBPS = 6.29        # float4 copy on this chip (microarchitecture notes)


class LegTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise LegTimeout()


def median_ms(fn, reps, warm=2):
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
    return float(np.median(ms))


def torch_copy(srcs, flip, work):
    """What the front end did with a time-major device tensor: permute, flip, cast, contiguous -- field by field."""
    outs = []
    for s in srcs:
        v = s.permute(2, 1, 0)
        if flip:
            v = torch.flip(v, dims=(1,))
        outs.append(v.to(dtype=work).contiguous())
    return outs


def kernel_leg(name, ne, nlev, nt, dtype, reps):
    ncol = synth.ncol_of_ne(ne)
    g = torch.Generator(device=DEV).manual_seed(1)
    srcs = [torch.randn((nt, nlev, ncol), generator=g, device=DEV, dtype=dtype) for _ in range(4)]
    rows = []
    variants = [("plain", False, dtype), ("flip", True, dtype)]
    if dtype == torch.float32:
        variants.append(("widen", False, torch.float64))
    for vname, flip, work in variants:
        # both sides alike: outputs allocated inside the timed call, the same warm-ups and repetitions
        t_k = median_ms(lambda: layout.to_engine_layout(srcs, flip_lev=flip, dtype=work), reps)
        out = layout.to_engine_layout(srcs[:1], flip_lev=flip, dtype=work)[0]
        ref = torch_copy(srcs[:1], flip, work)[0]
        same = bool(torch.equal(out, ref))
        del ref, out
        t_t = median_ms(lambda: torch_copy(srcs, flip, work), reps)
        nbytes = 4 * ncol * nlev * nt * (srcs[0].element_size() + torch.empty((), dtype=work).element_size())
        rec = {"leg": name, "variant": vname, "ncol": ncol, "nlev": nlev, "nt": nt,
               "src_dtype": str(dtype).replace("torch.", ""), "dst_dtype": str(work).replace("torch.", ""), "nf": 4,
               "bytes_read_plus_written": nbytes, "relayout_ms": round(t_k, 4), "torch_ms": round(t_t, 4),
               "relayout_TBps": round(nbytes / t_k / 1e9, 3), "fraction_of_float4_copy": round(nbytes / t_k / 1e9 / COPY_TBPS, 3),
               "torch_over_relayout_time": round(t_t / t_k, 2), "equal_to_torch": same}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        torch.cuda.empty_cache()
    return rows


def blocked_leg(nt, time_block, parent_nt):
    from pytemdiags_amd import TEMDiagnostics
    ne, nlev = 30, 72
    lat, lon = synth.cubed_sphere_gll(ne)
    plev = synth.pressure_levels(nlev)
    ncol = lat.size
    # a host-resident time-major record: synthetic fields of a few snapshots, tiled along time with a drift
    base = [np.ascontiguousarray(np.transpose(x, (2, 1, 0))) for x in
            synth.analytic_fields(lat, lon, plev, 8, seed=3, dtype=np.float32)]
    host = [np.empty((nt, nlev, ncol), dtype=np.float32) for _ in range(4)]
    for h, b in zip(host, base):
        for t in range(0, nt, 8):
            n = min(8, nt - t)
            h[t:t + n] = b[:n] * np.float32(1.0 + 1e-3 * (t // 8))
    kw = dict(plev=plev, dims=("time", "plev", "ncol"), debug_level=0)
    TEMDiagnostics(*[h[:2 * time_block] for h in host], lat, time_block=time_block, **kw)      # warm-up: plan, tables
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tem = TEMDiagnostics(*host, lat, time_block=time_block, **kw)
    torch.cuda.synchronize()
    t_blocked = time.perf_counter() - t0
    tm = tem.block_timing
    rec = {"leg": "blocked_constructor", "ncol": int(ncol), "nlev": nlev, "nt": nt, "dtype": "float32",
           "time_block": time_block, "blocks": len(tm["upload_ms"]), "record_bytes": int(4 * nt * nlev * ncol * 4),
           "blocked_s": round(t_blocked, 3), "blocked_s_per_snapshot": round(t_blocked / nt, 5),
           "per_block_ms": {k: {"median": round(float(np.median(v)), 3), "sum": round(float(np.sum(v)), 1)}
                            for k, v in tm.items()}}
    # the whole run without the re-layout, on the prefix it can hold: host-side permute + contiguous, pageable upload
    pn = min(parent_nt, nt)
    keep = layout.is_time_major
    layout.is_time_major = lambda *a: False
    try:
        t0 = time.perf_counter()
        ref = TEMDiagnostics(*[h[:pn] for h in host], lat, **kw)
        torch.cuda.synchronize()
        t_parent = time.perf_counter() - t0
    finally:
        layout.is_time_major = keep
    assert ref.input_path == "torch"
    err = float((tem._res[..., :pn] - ref._res).abs().max() / ref._res.abs().max())
    rec.update({"parent_prefix_nt": pn, "parent_s": round(t_parent, 3), "parent_s_per_snapshot": round(t_parent / pn, 5),
                "parent_over_blocked_per_snapshot": round((t_parent / pn) / (t_blocked / nt), 2),
                "max_rel_diff_on_prefix": err})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nt", type=int, default=730)
    ap.add_argument("--time-block", type=int, default=32)
    ap.add_argument("--parent-nt", type=int, default=92)
    ap.add_argument("--skip-blocked", action="store_true")
    ap.add_argument("--leg-limit", type=int, default=240, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--out", default="profiles/relayout_bench_mi355x.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "relayout_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "float4_copy_TBps": COPY_TBPS, "legs": []}
    legs = [("ne120x72x30_f64", lambda: kernel_leg("ne120x72x30_f64", 120, 72, 30, torch.float64, a.reps)),
            ("ne120x72x30_f32", lambda: kernel_leg("ne120x72x30_f32", 120, 72, 30, torch.float32, a.reps)),
            ("ne30x72x92_f64", lambda: kernel_leg("ne30x72x92_f64", 30, 72, 92, torch.float64, a.reps))]
    if not a.skip_blocked:
        legs.append(("blocked_constructor", lambda: [blocked_leg(a.nt, a.time_block, a.parent_nt)]))
    rc = 0
    for name, fn in legs:
        signal.alarm(a.leg_limit)
        try:
            rec["legs"] += fn()
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
