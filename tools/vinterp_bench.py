#!/usr/bin/env python3
"""Timing of temxv_interp (model levels -> pressure levels, include/temx_vert.h), one process.

Cases: hybrid pressure, log interpolation, 4 fields -> the 37 standard levels on
  ne120 x 72 x 30 fp64, ne30 x 72 x 91 fp64, ne30 x 72 x 1 fp64, ne240 x 128 x 1 fp32.
Each case, in this process: the median of --reps runs after a warm-up (HIP events) of
  * temxv_interp, and
  * a torch device copy that moves the same number of bytes (the fields read, plus ps, plus the outputs written):
    the yardstick, measured here rather than assumed;
and their ratio.  At ne30 x 72 x 91 the same interpolation written with plain torch ops (searchsorted + gather), which
is what a user would otherwise write, is timed too.  --switch adds the lane-map A/B: both maps (TEMXV_MAP=time / slab)
over a range of row lengths, the measurement the switch point of the two maps rests on.

  python tools/vinterp_bench.py [--reps 20 --switch --out profiles/vinterp_bench.json]
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

PLEV37 = np.array([1, 2, 3, 5, 7, 10, 20, 30, 50, 70, 100, 125, 150, 175, 200, 225, 250, 300, 350, 400, 450, 500, 550,
                   600, 650, 700, 750, 775, 800, 825, 850, 875, 900, 925, 950, 975, 1000], dtype=np.float64)
DEV = torch.device("cuda", 0)


def hybrid_levels(nlev):
    eta = np.exp(np.linspace(np.log(1e-4), np.log(0.9976), nlev))
    b = np.maximum((eta - 0.2) / 0.8, 0.0) ** 1.3
    return eta - b, b


def surface_pressure(ncol, nt):
    """1e5 +- 1500 Pa with longitude-like phase and time, a cap at 6.5e4 and a plateau at 6e4 (the fixture of
    tests/test_vertical_host.py, by column index instead of a grid: only the values matter here)."""
    i = torch.arange(ncol, device=DEV, dtype=torch.float64)[:, None]
    t = torch.arange(nt, device=DEV, dtype=torch.float64)[None, :]
    ps = 1e5 + 1500.0 * torch.sin(i * 0.0137 + 0.7 * t) * torch.cos(i * 1e-5)
    ps = torch.where(i % 97 == 0, torch.full_like(ps, 6.5e4), ps)
    return torch.where(i % 89 == 0, torch.full_like(ps, 6.0e4), ps).contiguous()


def median_ms(fn, reps, warm=3):
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


def make(ncol, nlev, nt, dtype, nf=4):
    g = torch.Generator(device=DEV).manual_seed(1)
    f = [torch.randn((ncol, nlev, nt), generator=g, device=DEV, dtype=dtype) for _ in range(nf)]
    return f, surface_pressure(ncol, nt)


def run_interp(f, ps, hyam, hybm):
    return vertical.interp_device(f, PLEV37 * 100.0, ps=ps, hyam=hyam, hybm=hybm, p0=1e5, method="log", edge="nan")


def bytes_moved(f, ps):
    ncol, nlev, nt = f[0].shape
    sz = f[0].element_size()
    return len(f) * ncol * nt * (nlev + PLEV37.size) * sz + ps.numel() * ps.element_size()


def torch_interp(f, ps, hyam, hybm):
    """The same contract (log, edge = nan) with searchsorted + gather."""
    nlev = f[0].shape[1]
    a = torch.as_tensor(hyam, device=DEV)[None, None, :]
    b = torch.as_tensor(hybm, device=DEV)[None, None, :]
    p = a * 1e5 + b * ps[:, :, None]                                   # [ncol][nt][nlev]
    x = torch.log(p)
    pt = torch.as_tensor(PLEV37 * 100.0, device=DEV)
    xt = torch.log(pt)[None, None, :].expand(p.shape[0], p.shape[1], -1).contiguous()
    idx = torch.searchsorted(x, xt).clamp(1, nlev - 1)
    x0, x1 = torch.gather(x, 2, idx - 1), torch.gather(x, 2, idx)
    w = (xt - x0) / (x1 - x0)
    outside = (pt[None, None, :] < p[:, :, :1]) | (pt[None, None, :] > p[:, :, -1:])
    outs = []
    for v in f:
        vt = v.permute(0, 2, 1).to(torch.float64)
        y0, y1 = torch.gather(vt, 2, idx - 1), torch.gather(vt, 2, idx)
        y = torch.where(outside, torch.full_like(y0, float("nan")), y0 + w * (y1 - y0))
        outs.append(y.permute(0, 2, 1).to(v.dtype).contiguous())
    return outs


def case(name, ne, nlev, nt, dtype, reps, with_torch=False):
    ncol = synth.ncol_of_ne(ne)
    hyam, hybm = hybrid_levels(nlev)
    f, ps = make(ncol, nlev, nt, dtype)
    nbytes = bytes_moved(f, ps)
    t_k = median_ms(lambda: run_interp(f, ps, hyam, hybm), reps)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    t_c = median_ms(lambda: dst.copy_(src), reps)
    del src, dst
    rec = {"case": name, "ncol": ncol, "nlev": nlev, "nt": nt, "dtype": str(dtype).replace("torch.", ""), "nf": 4,
           "nplev": int(PLEV37.size), "bytes": nbytes, "interp_ms": round(t_k, 4), "copy_ms": round(t_c, 4),
           "interp_TBps": round(nbytes / t_k / 1e9, 3), "copy_TBps": round(nbytes / t_c / 1e9, 3),
           "interp_over_copy_time": round(t_k / t_c, 3)}
    if with_torch:
        ref = torch_interp(f, ps, hyam, hybm)
        out = run_interp(f, ps, hyam, hybm)
        err = max(float(torch.nan_to_num(a - b).abs().max()) for a, b in zip(out, ref))
        same = all(bool((torch.isnan(a) == torch.isnan(b)).all()) for a, b in zip(out, ref))
        del ref, out
        t_t = median_ms(lambda: torch_interp(f, ps, hyam, hybm), max(3, reps // 4), warm=1)
        rec.update({"torch_ops_ms": round(t_t, 3), "torch_over_interp_time": round(t_t / t_k, 1),
                    "torch_ops_max_abs_diff": err, "torch_ops_same_nan_pattern": same})
    print(json.dumps(rec), flush=True)
    return rec


def switch_sweep(reps):
    """Both lane maps over row lengths, ne30 x 72, 4 fields: time per (column, time) pair."""
    rows = []
    ncol = synth.ncol_of_ne(30)
    hyam, hybm = hybrid_levels(72)
    for dtype in (torch.float64, torch.float32):
        for nt in (1, 2, 4, 8, 12, 16, 24, 32):
            f, ps = make(ncol, 72, nt, dtype)
            rec = {"dtype": str(dtype).replace("torch.", ""), "nt": nt, "row_bytes": nt * f[0].element_size()}
            for m in ("time", "slab"):
                os.environ["TEMXV_MAP"] = m
                try:
                    rec[m + "_ms"] = round(median_ms(lambda: run_interp(f, ps, hyam, hybm), reps), 4)
                except Exception as e:  # noqa: BLE001  (the slab map refuses shapes whose column does not fit LDS)
                    rec[m + "_ms"] = None
                    rec[m + "_error"] = str(e)[:80]
            os.environ.pop("TEMXV_MAP", None)
            rec["TBps_time"] = round(bytes_moved(f, ps) / rec["time_ms"] / 1e9, 3)
            if rec["slab_ms"]:
                rec["TBps_slab"] = round(bytes_moved(f, ps) / rec["slab_ms"] / 1e9, 3)
            print(json.dumps(rec), flush=True)
            rows.append(rec)
            del f, ps
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--switch", action="store_true", help="also time both lane maps over a range of row lengths")
    ap.add_argument("--only", default=None, help="run one case by name (for a kernel trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the process ends itself")
    a = ap.parse_args()
    signal.alarm(a.time_limit)
    assert torch.cuda.is_available(), "vinterp_bench needs a GPU"
    cases = [("ne30x72x1_f64", 30, 72, 1, torch.float64, False),
             ("ne30x72x91_f64", 30, 72, 91, torch.float64, True),
             ("ne240x128x1_f32", 240, 128, 1, torch.float32, False),
             ("ne120x72x30_f64", 120, 72, 30, torch.float64, False)]
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": []}
    for name, ne, nlev, nt, dtype, wt in cases:
        if a.only and a.only != name:
            continue
        rec["cases"].append(case(name, ne, nlev, nt, dtype, a.reps, with_torch=wt))
        torch.cuda.empty_cache()
    if a.switch:
        rec["lane_map_switch"] = switch_sweep(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
