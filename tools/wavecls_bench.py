#!/usr/bin/env python3
"""Timing of the class form of the zonal-wavenumber fit (temxz_wave_fluxes, pytemdiags_amd/include_wavecls/temx_wavecls.h)
beside the generic form (temxk_wave_fluxes, the yardstick: existing code) and ``temx_tem_run``, one process, a time limit
per leg.  (The per-leg limit is an alarm the interpreter answers between calls; a leg stuck inside a blocking device call
is ended only from outside: run the tool under ``timeout -k 10 <seconds>``.)

Legs: ne120 x 72 x 30, fp64 and fp32 fields, L = 50, wavenumbers (1, 2, 3); for the record ne30 x 72 x 91 and a lat-lon
grid of 360 x 720 x 72 x 2 (fp64).  Recorded per leg, as the median and min-max of --reps runs after --warm warm-ups, from
HIP events (and a host clock around a synchronise):
  * ``temx_tem_run`` of the same process;
  * the generic call end to end (with the parts) and its projection sweeps alone (the events of ``temxk_wave_timing``:
    sweep and slab reduction of each wavenumber, summed per call), hence per m;
  * the class call end to end (with the parts).  Its sweeps alone are the call less what the two forms share -- the solve
    and the flux kernel, the generic call less the generic sweeps -- hence per m; the ratio class sweep / generic sweep and
    the generic sweep's own (max - min) / median next to it;
  * a copy of the four fields' bytes (``Tensor.copy_`` of one field-sized buffer, times four; vector loads and stores of 16
    bytes) and the read rate of the class sweep (field bytes over its time) against the copy's read + write rate;
  * the device bytes both states hold after creation and after the calls, and their build times.

  python tools/wavecls_bench.py [--reps 20 --warm 3 --out profiles/wavecls_bench_mi355x.json]
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pytemdiags_amd import _lib, _wavecls, engine, synth, waves  # noqa: E402


class LegTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise LegTimeout()


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def stats_ms(fn, reps, warm, extra=None):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    if extra is not None:
        extra()                      # (drops what the warm-ups recorded)
    ev, wall, ex = [], [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
        if extra is not None:
            ex.append(extra())
    out = {"event_ms": summary(ev), "wall_ms": summary(wall)}
    if extra is not None:
        out["extra"] = summary(ex)
    return out


def sweep_timer(state):
    """Switch the sweep events of the generic ``state`` on; -> the reader for ``stats_ms``."""
    lib = state.lib

    def read():
        ms, n = C.c_double(0), C.c_int(0)
        _lib.check(lib.temxk_wave_timing_read(state._h, C.byref(ms), C.byref(n)))
        _lib.check(lib.temxk_wave_timing(state._h, 1))
        return ms.value
    _lib.check(lib.temxk_wave_timing(state._h, 1))
    return read


def leg(name, grid, nlev, nt, dtype, L, ms, reps, warm):
    lat, lon = synth.cubed_sphere_gll(grid) if isinstance(grid, int) else synth.latlon_grid(*grid)
    plev = synth.pressure_levels(nlev)
    ncol, D = lat.size, nlev * nt
    fields = engine.synth_fields(0, lat, lon, plev, nt, dtype=dtype, seed=7)
    lat_out = np.arange(-89.5, 90, 1.0)
    plan = engine.Plan(lat, lat_out, L, device=0, fp32_fields=dtype == torch.float32)
    plan.set_tem(nlev, nt, plev * 100)
    out = plan._alloc_results(True)
    run = stats_ms(lambda: plan.tem_run(*fields, out=out), reps, warm)
    nm = len(ms)
    # the yardstick: the generic form
    t0 = time.perf_counter()
    gen = waves.WaveState(plan, lon, ms)
    torch.cuda.synchronize()
    gen_build = time.perf_counter() - t0
    gen_bytes0 = gen.workspace_bytes
    read = sweep_timer(gen)
    gflux = stats_ms(lambda: gen.fluxes(*fields, want_parts=True), reps, warm, extra=read)
    gsweeps = gflux.pop("extra")
    gen_bytes1 = gen.workspace_bytes
    gref = gen.fluxes(*fields, want_parts=True)
    gen.close()
    torch.cuda.empty_cache()
    # the class form
    t0 = time.perf_counter()
    cls = waves.WaveState(plan, lon, ms, form="classes")
    torch.cuda.synchronize()
    cls_build = time.perf_counter() - t0
    cls_bytes0 = cls.workspace_bytes
    cflux = stats_ms(lambda: cls.fluxes(*fields, want_parts=True), reps, warm)
    cls_bytes1 = cls.workspace_bytes
    cref = cls.fluxes(*fields, want_parts=True)
    launch = cls.launch(ms[0], 4, D)
    assert not cls.status()
    cls.close()
    agree = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(cref, gref))
    del cref, gref
    # a copy of one field's bytes, times four
    src = fields[0].reshape(-1)
    dst = torch.empty_like(src)
    copy = stats_ms(lambda: dst.copy_(src), reps, warm)["event_ms"]
    del dst
    plan.close()
    field_bytes = 4.0 * ncol * D * fields[0].element_size()
    shared = gflux["event_ms"]["median"] - gsweeps["median"]                  # solve + flux kernels of the nm wavenumbers
    csweeps = cflux["event_ms"]["median"] - shared
    rec = {"leg": name, "ncol": int(ncol), "nlev": nlev, "nt": nt, "dtype": str(dtype).replace("torch.", ""), "L": L,
           "wavenumbers": list(ms), "class_shape": [_wavecls.shape(L, m) for m in ms], "class_launch_nf4": launch,
           "tem_run_ms": run,
           "generic_fluxes_ms": gflux, "generic_sweeps_ms_per_call": gsweeps,
           "generic_sweep_ms_per_m": round(gsweeps["median"] / nm, 4),
           "generic_sweep_spread_over_median": round((gsweeps["max"] - gsweeps["min"]) / gsweeps["median"], 4),
           "class_fluxes_ms": cflux, "shared_tail_ms_per_call": round(shared, 4),
           "class_sweeps_ms_per_call_derived": round(csweeps, 4), "class_sweep_ms_per_m_derived": round(csweeps / nm, 4),
           "class_sweep_over_generic_sweep": round(csweeps / gsweeps["median"], 4),
           "class_fluxes_over_generic_fluxes": round(cflux["event_ms"]["median"] / gflux["event_ms"]["median"], 4),
           "class_sweep_over_tem_run": round(csweeps / nm / run["event_ms"]["median"], 4),
           "copy_of_one_field_ms": copy, "copy_read_plus_write_TBps": round(2.0 * field_bytes / 4 / copy["median"] / 1e9, 3),
           "class_sweep_field_read_TBps": round(field_bytes / (csweeps / nm) / 1e9, 3),
           "generic_sweep_field_read_TBps": round(field_bytes / (gsweeps["median"] / nm) / 1e9, 3),
           "generic_state_bytes": {"after_create": int(gen_bytes0), "after_calls": int(gen_bytes1)},
           "class_state_bytes": {"after_create": int(cls_bytes0), "after_calls": int(cls_bytes1)},
           "generic_state_build_s": round(gen_build, 3), "class_state_build_s": round(cls_build, 3),
           "forms_agree_to": float("%.3g" % agree)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--leg-limit", type=int, default=240, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--small", action="store_true", help="ne30 x 8 x 4 only: a run to see that the tool works")
    ap.add_argument("--out", default="profiles/wavecls_bench_mi355x.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "wavecls_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm, "legs": []}
    legs = [("ne120x72x30_f64", 120, 72, 30, torch.float64), ("ne120x72x30_f32", 120, 72, 30, torch.float32),
            ("ne30x72x91_f64", 30, 72, 91, torch.float64), ("latlon360x720x72x2_f64", (360, 720), 72, 2, torch.float64)]
    if a.small:
        legs = [("ne30x8x4_f64", 30, 8, 4, torch.float64)]
    rc = 0
    for n, grid, nlev, nt, dt in legs:
        signal.alarm(a.leg_limit)
        try:
            rec["legs"].append(leg(n, grid, nlev, nt, dt, a.L, (1, 2, 3), a.reps, a.warm))
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
