#!/usr/bin/env python3
"""Timing of the zonal-wavenumber fluxes (temxk_wave_fluxes, pytemdiags_amd/include/temx_wave.h), one process, a time
limit per leg.  (The per-leg limit is an alarm the interpreter answers between calls; a leg stuck inside a blocking device
call is ended only from outside: run the tool under ``timeout -k 10 <seconds>``.)

Legs: ne120 x 72 x 30, fp64 and fp32 fields, L = 50, wavenumbers (1, 2, 3) (Kc = 100, 98, 96).  Recorded per leg, as the
median and min-max of --reps runs after --warm warm-ups, from HIP events and from a host clock around a synchronise:
  * ``temxk_wave_fluxes`` (with the parts), and its projection sweeps alone (the events of ``temxk_wave_timing``: sweep
    and slab reduction of each wavenumber, summed per call), beside the plain ``temx_tem_run`` of the same process;
  * the build time of the wave state (``temxk_wave_create``, host clock) and its workspace;
  * the yardstick of the sweep: the project's own generic projection at equal width, ``temx_project`` of an L = 99 plan
    without symmetry (K = 100 = Kc of m = 1) on the same four fields in the same process, beside the time of the m = 1
    sweep alone (a state of one wavenumber).  Both stream a basis of 100 columns against the same bytes;
  * the fp64 MFMA rate of the m = 1 sweep, 2 ncol Kc D 4 useful floating-point operations over its time, against
    ``temx_mfma_f64_peak`` measured in the same process.

  python tools/wave_bench.py [--reps 20 --warm 3 --out profiles/wave_bench_mi355x.json]
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

from pytemdiags_amd import _lib, _wave, engine, synth, waves  # noqa: E402

DEV = torch.device("cuda", 0)


class LegTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise LegTimeout()


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def stats_ms(fn, reps, warm, extra=None):
    """-> {"event_ms": ..., "wall_ms": ...} (and what ``extra()`` returns after each run, summarised)."""
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
    """Switch the sweep events of ``state`` on; -> (reset, read) for ``stats_ms``."""
    lib = state.lib

    def reset():
        _lib.check(lib.temxk_wave_timing(state._h, 1))

    def read():
        ms, n = C.c_double(0), C.c_int(0)
        _lib.check(lib.temxk_wave_timing_read(state._h, C.byref(ms), C.byref(n)))
        reset()
        return ms.value
    reset()
    return reset, read


def leg(name, ne, nlev, nt, dtype, L, ms, reps, warm, peak):
    lat, lon = synth.cubed_sphere_gll(ne)
    plev = synth.pressure_levels(nlev)
    ncol, D = lat.size, nlev * nt
    fields = engine.synth_fields(0, lat, lon, plev, nt, dtype=dtype, seed=7)
    lat_out = np.arange(-89.5, 90, 1.0)
    plan = engine.Plan(lat, lat_out, L, device=0, fp32_fields=dtype == torch.float32)
    plan.set_tem(nlev, nt, plev * 100)
    out = plan._alloc_results(True)
    run = stats_ms(lambda: plan.tem_run(*fields, out=out), reps, warm)
    t0 = time.perf_counter()
    state = waves.WaveState(plan, lon, ms)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    _, read = sweep_timer(state)
    flux = stats_ms(lambda: state.fluxes(*fields, want_parts=True), reps, warm, extra=read)
    workspace = state.workspace_bytes
    state.close()
    # the m = 1 sweep alone, and its yardstick: temx_project of a generic L = Kc - 1 plan on the same fields
    one = waves.WaveState(plan, lon, ms[:1])
    _, read1 = sweep_timer(one)
    one_sweep = stats_ms(lambda: one.fluxes(*fields), reps, warm, extra=read1)["extra"]
    one.close()
    kc = _wave.kc(L, ms[0])
    wide = engine.Plan(lat, lat_out, kc - 1, device=0, symmetry=False, fp32_fields=dtype == torch.float32)
    assert wide.sweep_mode == 0
    yard = stats_ms(lambda: [wide.project(x) for x in fields], reps, warm)["event_ms"]
    wide.close()
    plan.close()
    spread = yard["max"] - yard["min"]
    ratio = one_sweep["median"] / yard["median"]
    flops = 2.0 * ncol * kc * D * 4
    rec = {"leg": name, "ncol": int(ncol), "nlev": nlev, "nt": nt, "dtype": str(dtype).replace("torch.", ""), "L": L,
           "wavenumbers": list(ms), "Kc": [_wave.kc(L, m) for m in ms],
           "tem_run_ms": run, "wave_fluxes_ms": flux, "wave_sweeps_ms_per_call": flux.pop("extra"),
           "wave_state_build_s": round(build_s, 3), "wave_workspace_bytes": int(workspace),
           "stored_basis_bytes_per_m": [int(ncol) * _wave.shape(L, m)["kpad"] * 8 for m in ms],
           "field_reads_per_call": sum(_wave.shape(L, m)["nslice"] for m in ms),
           "sweep_m%d_ms" % ms[0]: one_sweep,
           "yardstick": "temx_project x 4 fields, generic plan L = %d (K = %d)" % (kc - 1, kc), "yardstick_ms": yard,
           "sweep_over_yardstick": round(ratio, 3), "yardstick_spread_over_median": round(spread / yard["median"], 3),
           "sweep_useful_fp64_tflops": round(flops / one_sweep["median"] / 1e9, 2), "mfma_f64_peak_tflops": round(peak, 2),
           "sweep_share_of_mfma_peak": round(flops / one_sweep["median"] / 1e9 / peak, 3),
           "sweep_field_bytes_TBps": round(4.0 * ncol * D * fields[0].element_size() / one_sweep["median"] / 1e9, 3)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--ne", type=int, default=120)
    ap.add_argument("--nlev", type=int, default=72)
    ap.add_argument("--nt", type=int, default=30)
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--leg-limit", type=int, default=240, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--out", default="profiles/wave_bench_mi355x.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "wave_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    peak = engine.mfma_f64_peak(0)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm, "legs": []}
    rc = 0
    for dt in (torch.float64, torch.float32):
        n = "ne%dx%dx%d_%s" % (a.ne, a.nlev, a.nt, "f64" if dt == torch.float64 else "f32")
        signal.alarm(a.leg_limit)
        try:
            rec["legs"].append(leg(n, a.ne, a.nlev, a.nt, dt, a.L, (1, 2, 3), a.reps, a.warm, peak))
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
