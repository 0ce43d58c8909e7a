#!/usr/bin/env python3
"""Timing of temxf_filter_time (the time filter of fields in engine layout, pytemdiags_amd/include/temx_tfilt.h) and of
the constructor with and without ``time_bands=``, one process, a time limit per leg.  (The per-leg limit is an alarm the
interpreter answers between calls; a leg stuck inside a blocking device call is ended only from outside: run the tool
under ``timeout -k 10 <seconds>``.)

Filter legs, 4 fields: ne30 x 72 x 730 fp64 and fp32 and ne120 x 72 x 120 fp32, each with nw = 31 and 121 weights and
nb = 1 and 2 bands (ne120 x 72 x 120 holds no window of 121 weights: those legs are recorded as not applicable), each
against the torch composition on the same tensors: ``unfold`` + ``matmul`` for both dtypes, in chunks of columns so that
the unfolded copy stays at 2^28 elements; it is timed on one field and that time taken four times.  (``conv1d`` on the
``[rows][1][nt]`` view with the ``[nb][1][nw]`` kernel has no fp64 path, and the one fp32 leg that went through it, ne30 x 72 x 730
with 31 weights, did not finish within its 180 s on the MI355X; ``--conv1d`` takes that path again.)  Reported: median ms of --reps runs after --warm warm-ups (HIP events), bytes moved per
second counting one read of the record plus nb writes, that rate as a fraction of the rate of ``dst.copy_(src)`` on 4 GiB
of fp32 measured in this process (bytes read + written per second), and the ratio to torch.

Constructor leg: ``TEMDiagnostics`` on device-resident ne30 x 72 x 240 fp64 fields with and without two bands of 31
weights, wall time, interleaved.

  python tools/tfilt_bench.py [--reps 20 --warm 3 --out profiles/tfilt_bench_mi355x.json]
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

from pytemdiags_amd import _tfilt, engine, synth, timebands  # noqa: E402

DEV = torch.device("cuda", 0)
CONV1D = False          # --conv1d: the fp32 legs through torch.nn.functional.conv1d


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


def torch_filter(x, w, out):
    """The torch composition for one field ``[ncol][nlev][nt]`` and the weights ``[nb][nw]`` of x's dtype -> ``out``
    ``[nb][ncol][nlev][nto]``."""
    ncol, nlev, nt = x.shape
    nb, nw = w.shape
    if CONV1D and x.dtype == torch.float32:
        y = torch.nn.functional.conv1d(x.view(ncol * nlev, 1, nt), w.view(nb, 1, nw))       # [rows][nb][nto]
        out.copy_(y.view(ncol, nlev, nb, nt - nw + 1).permute(2, 0, 1, 3))
        return
    step = max(1, (1 << 28) // (nlev * (nt - nw + 1) * nw))                                 # columns per chunk
    for c0 in range(0, ncol, step):
        u = x[c0:c0 + step].unfold(-1, nw, 1)                                              # [c][nlev][nto][nw] view
        out[:, c0:c0 + step] = torch.matmul(u, w.t()).permute(3, 0, 1, 2)


def filter_leg(name, ne, nlev, nt, dtype, nw, nb, reps, warm, copy_tbps):
    ncol = synth.ncol_of_ne(ne)
    esz = 4 if dtype == torch.float32 else 8
    base = {"leg": name, "ncol": ncol, "nlev": nlev, "nt": nt, "dtype": str(dtype).replace("torch.", ""), "nf": 4, "nw": nw, "nb": nb}
    if nt < nw:
        rec = dict(base, not_applicable="nt < nw: the record holds no window of this filter")
        print(json.dumps(rec), flush=True)
        return rec
    nto = nt - nw + 1
    g = torch.Generator(device=DEV).manual_seed(1)
    fields = [torch.randn((ncol, nlev, nt), generator=g, device=DEV, dtype=dtype) for _ in range(4)]
    wnp = np.stack([timebands.lanczos(nw, low=0.1 + 0.1 * b) for b in range(nb)])
    w64 = torch.tensor(wnp, device=DEV)
    outs = [torch.empty((nb, ncol, nlev, nto), dtype=dtype, device=DEV) for _ in range(4)]
    lib = _tfilt.load()
    src = (C.c_void_p * 4)(*[x.data_ptr() for x in fields])
    dts = (C.c_int * 4)(*[engine._DT[dtype]] * 4)
    dst = (C.c_void_p * (nb * 4))(*[outs[f][b].data_ptr() for b in range(nb) for f in range(4)])

    def kernel():
        st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        _tfilt.check(lib.temxf_filter_time(0, 4, src, dts, nb, dst, engine._DT[dtype], ncol, nlev, nt, nw,
                                           C.c_void_p(w64.data_ptr()), 0, st))
    k = stats_ms(kernel, reps, warm)
    got = outs[0][:, :64].clone()
    wt = w64.to(dtype)
    tout = outs[1]            # (the kernel's timing is done: the torch composition writes over its second output)
    # one field is timed and the time taken four times: the composition has no call for several fields
    t = tuple(4 * v for v in stats_ms(lambda: torch_filter(fields[0], wt, tout), max(3, reps // 4), 1))
    delta = float((got.double() - tout[:, :64].double()).abs().max())
    nbytes = 4 * ncol * nlev * (nt + nb * nto) * esz
    rec = dict(base, cut=_tfilt.shape(ncol * nlev, nt, nw, nb, esz, esz), bytes_moved=nbytes, taps_per_element=nw * nb,
               kernel_ms=round(k[0], 4), kernel_ms_min_max=[round(k[1], 4), round(k[2], 4)],
               torch_ms=round(t[0], 4), torch_ms_min_max=[round(t[1], 4), round(t[2], 4)],
               torch_path="conv1d" if CONV1D and dtype == torch.float32 else "unfold+matmul",
               kernel_TBps=round(nbytes / k[0] / 1e9, 3), fraction_of_measured_copy=round(nbytes / k[0] / 1e9 / copy_tbps, 3),
               kernel_Gfma_per_s=round(4 * ncol * nlev * nto * nw * nb / k[0] / 1e6, 1),
               torch_over_kernel_time=round(t[0] / k[0], 3), max_abs_delta_vs_torch=delta)
    print(json.dumps(rec), flush=True)
    return rec


def constructor_leg(reps):
    from pytemdiags_amd import TEMDiagnostics
    ne, nlev, nt = 30, 72, 240      # (the whole-year record and its two filtered copies do not fit next to a TEM run)
    lat, lon = synth.cubed_sphere_gll(ne)[:2]
    plev = synth.pressure_levels(nlev)
    fields = engine.synth_fields(0, lat, lon, plev, nt)
    kw = dict(plev=plev, debug_level=0)
    bands = {"synoptic": timebands.lanczos(31, low=0.4, high=0.125), "low": timebands.lanczos(31, low=0.1)}
    TEMDiagnostics(*fields, lat, time_bands=bands, **kw)            # warm-up: plan tables, allocator
    torch.cuda.synchronize()
    times = {False: [], True: []}
    ws = 0
    for _ in range(reps):
        for on in (False, True):
            t0 = time.perf_counter()
            tem = TEMDiagnostics(*fields, lat, time_bands=bands if on else None, **kw)
            torch.cuda.synchronize()
            times[on].append(time.perf_counter() - t0)
            ws = tem.bands.workspace_bytes if on else ws
            del tem
    rec = {"leg": "constructor", "ncol": int(lat.size), "nlev": nlev, "nt": nt, "dtype": "float64", "reps": reps, "nb": 2, "nw": 31,
           "plain_s": round(float(np.median(times[False])), 4), "plain_s_min_max": [round(min(times[False]), 4), round(max(times[False]), 4)],
           "time_bands_s": round(float(np.median(times[True])), 4),
           "time_bands_s_min_max": [round(min(times[True]), 4), round(max(times[True]), 4)], "workspace_bytes": int(ws)}
    rec["time_bands_over_plain"] = round(rec["time_bands_s"] / rec["plain_s"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--constructor-reps", type=int, default=3)
    ap.add_argument("--skip-constructor", action="store_true")
    ap.add_argument("--only", default="", help="run the filter legs whose name holds this text")
    ap.add_argument("--conv1d", action="store_true", help="fp32 legs: conv1d as the torch composition")
    ap.add_argument("--leg-limit", type=int, default=180, help="seconds a leg may take; the process ends at the first leg over it")
    ap.add_argument("--out", default="profiles/tfilt_bench_mi355x.json")
    a = ap.parse_args()
    global CONV1D
    CONV1D = a.conv1d
    assert torch.cuda.is_available(), "tfilt_bench needs a GPU"
    signal.signal(signal.SIGALRM, _alarm)
    copy_tbps = float4_copy_TBps(a.reps, a.warm)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": a.warm,
           "float4_copy_TBps_measured": round(copy_tbps, 3), "filter": [], "constructor": None}
    print(json.dumps({"float4_copy_TBps_measured": rec["float4_copy_TBps_measured"]}), flush=True)
    shapes = [("ne30x72x730_f64", 30, 72, 730, torch.float64), ("ne30x72x730_f32", 30, 72, 730, torch.float32),
              ("ne120x72x120_f32", 120, 72, 120, torch.float32)]
    legs = []
    for n, ne, nl, nt, dt in shapes:
        for nw in (31, 121):
            for nb in (1, 2):
                if a.only not in "%s_nw%d_nb%d" % (n, nw, nb):
                    continue
                legs.append(("%s_nw%d_nb%d" % (n, nw, nb), (lambda n=n, ne=ne, nl=nl, nt=nt, dt=dt, nw=nw, nb=nb: rec["filter"].append(
                    filter_leg("%s_nw%d_nb%d" % (n, nw, nb), ne, nl, nt, dt, nw, nb, a.reps, a.warm, copy_tbps)))))
    if not a.skip_constructor:
        legs.append(("constructor", lambda: rec.__setitem__("constructor", constructor_leg(a.constructor_reps))))
    status = 0
    for name, leg in legs:
        signal.alarm(a.leg_limit)
        try:
            leg()
        except LegTimeout:
            print(json.dumps({"leg": name, "error": "time limit of %d s" % a.leg_limit}), flush=True)
            status = 1
            break
        finally:
            signal.alarm(0)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
