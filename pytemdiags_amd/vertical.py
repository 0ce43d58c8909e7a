"""Model levels to pressure levels on the GPU (include/temx_vert.h, kernels_vert.hpp).

The TEM engine takes fields on pressure levels.  Native model output lives on hybrid sigma-pressure levels,
``p = hyam * p0 + hybm * ps``, different in every column and at every time: ``interp_to_pressure`` is the vertical
remap in front of the engine, and ``TEMDiagnostics.from_model_levels`` chains the two.

This module validates, moves data and labels; the interpolation itself is one call of ``temxv_interp`` per eight
fields.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ingest, _vert, containers, layout

# Time-major model-level records (``records_to_pressure_device`` with ``path=None``): does the fused kernel
# (``temxi_records_to_pressure``) serve, per work dtype, or the chain of re-layout and interpolation?  The two give the
# same bits, so this is a matter of time alone: a dtype is switched on only by a measurement that shows the fused call
# no slower than the chain in every leg of that dtype of tools/ingest_bench.py, committed as
# profiles/ingest_bench_mi355x.json (tests/test_ingest_host.py holds the two together).  Measured, four fields: fp64
# 1.29 (ne120 x 72 -> 37 x 30), 1.06 (ne120 x 72 -> 72 x 16) and 1.14 (ne30 x 72 -> 37 x 92) times faster than the chain;
# fp32 0.86 at ne120 x 72 -> 37 x 30 -- slower: a level of its 32 x 32 tile takes a third of the LDS budget, so the level
# windows are one bracket long -- and stays off.
FUSED_RECORDS = {"float64": True, "float32": False}


def _values(x):
    return x.values if containers.is_labeled(x) else x


def _check_plev(plev_hpa):
    plev = np.atleast_1d(np.asarray(plev_hpa, dtype=np.float64))
    if plev.ndim != 1 or plev.size == 0:
        raise ValueError("plev_hpa must be a 1-d list of pressure levels in hPa")
    if not np.all(np.isfinite(plev)) or np.any(plev <= 0):
        raise ValueError("plev_hpa must be finite and positive")
    if plev.size > 1 and plev[0] > plev[-1]:
        plev = plev[::-1].copy()
    d = np.diff(plev)
    if np.any(d == 0):
        raise ValueError("plev_hpa has repeated levels")
    if np.any(d < 0):
        raise ValueError("plev_hpa must be sorted (ascending or descending)")
    return plev


def check_hybrid_monotone(hyam, hybm, p0, ps_min, ps_max):
    """p_k = hyam_k p0 + hybm_k ps is linear in ps, so it increases with k in every column exactly when it does at the
    smallest and at the largest surface pressure."""
    for ps in (ps_min, ps_max):
        pk = hyam * p0 + hybm * ps
        if not np.all(np.isfinite(pk)) or np.any(np.diff(pk) <= 0):
            k = int(np.argmax(~(np.diff(pk) > 0))) if pk.size > 1 else 0
            raise ValueError("hybrid levels are not strictly increasing in pressure at ps = %g Pa (levels %d, %d): "
                             "model levels must be ordered top first" % (ps, k, k + 1))


def _interp(fields, plev_hpa, *, ps=None, hyam=None, hybm=None, p0=1e5, p=None, method="log", edge="nan", device=None,
            on_device=False):
    """The work behind ``interp_to_pressure``.  Returns (outputs, ascending plev in hPa); with ``on_device`` the
    outputs keep device tensors as their values whatever kind came in (``from_model_levels`` feeds them on)."""
    import torch
    single = not isinstance(fields, (list, tuple))
    fl = [fields] if single else list(fields)
    # ---- everything that can be refused is refused before any device call ----
    if len(fl) == 0:
        raise ValueError("no fields given")
    if method not in _vert.METHODS:
        raise ValueError("method must be 'log' or 'linear', got %r" % (method,))
    if edge not in _vert.EDGES:
        raise ValueError("edge must be 'nan' or 'hold', got %r" % (edge,))
    if (ps is None) == (p is None):
        raise ValueError("give exactly one of ps= (hybrid levels, with hyam= and hybm=) and p= (pressure of every point)")
    hybrid = ps is not None
    if hybrid and (hyam is None or hybm is None):
        raise ValueError("hybrid levels (ps=) need hyam= and hybm=")
    plev = _check_plev(plev_hpa)
    labeled = [containers.is_labeled(x) for x in fl]
    if any(labeled) and not all(labeled):
        raise ValueError("fields must all be of the same kind")
    for x in fl:
        if not isinstance(_values(x), (np.ndarray, torch.Tensor)):
            raise ValueError("fields must be numpy arrays, torch tensors or labelled arrays of them")
    kind = "raw" if not labeled[0] else ("xarray" if containers.is_xarray(fl[0]) else "labeled")
    vals = [v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v)) for v in map(_values, fl)]
    shape = tuple(vals[0].shape)
    if len(shape) not in (2, 3):
        raise ValueError("fields must be [ncol][lev] or [ncol][lev][time], got %d dims" % len(shape))
    for i, v in enumerate(vals):
        if tuple(v.shape) != shape:
            raise ValueError("field %d has shape %s, expected %s" % (i, tuple(v.shape), shape))
        if not v.dtype.is_floating_point:
            raise ValueError("field %d is not a floating-point array" % i)
    two_d = len(shape) == 2
    ncol, nlev = shape[0], shape[1]
    nt = 1 if two_d else shape[2]
    if nlev < 2 or ncol < 1 or nt < 1:
        raise ValueError("fields need at least one column, two levels and one time, got shape %s" % (shape,))
    pin = _values(ps if hybrid else p)
    pin = pin if isinstance(pin, torch.Tensor) else torch.as_tensor(np.asarray(pin))
    if not pin.dtype.is_floating_point:
        pin = pin.to(torch.float64)
    want = ((ncol,) if two_d else (ncol, nt)) if hybrid else shape
    if tuple(pin.shape) != want and not (hybrid and nt == 1 and tuple(pin.shape) in ((ncol,), (ncol, 1))):
        raise ValueError("%s has shape %s, expected %s" % ("ps" if hybrid else "p", tuple(pin.shape), want))
    if hybrid:
        hyam = np.asarray(hyam, dtype=np.float64).ravel()
        hybm = np.asarray(hybm, dtype=np.float64).ravel()
        if hyam.shape[0] != nlev or hybm.shape[0] != nlev:
            raise ValueError("hyam / hybm have %d / %d entries but the fields have %d levels"
                             % (hyam.shape[0], hybm.shape[0], nlev))
        if not (np.all(np.isfinite(hyam)) and np.all(np.isfinite(hybm)) and np.isfinite(p0)):
            raise ValueError("hyam, hybm and p0 must be finite")
        fin = torch.isfinite(pin)        # a column without a surface pressure comes back NaN; it is no error
        if bool(fin.any()):
            lo = float(torch.where(fin, pin, torch.full_like(pin, float("inf"))).min())
            hi = float(torch.where(fin, pin, torch.full_like(pin, float("-inf"))).max())
            check_hybrid_monotone(hyam, hybm, float(p0), lo, hi)
    else:
        hyam = hybm = None

    # ---- device: contiguous [ncol][lev][time], one dtype; the model-level copies made here die with this frame ----
    work = torch.float32 if {v.dtype for v in vals} == {torch.float32} else torch.float64
    if device is None:
        device = vals[0].device.index if vals[0].is_cuda else 0
    dev = device if isinstance(device, torch.device) else torch.device("cuda", int(device))
    src = [v.reshape(ncol, nlev, nt).to(device=dev, dtype=work).contiguous() for v in vals]
    pdt = torch.float32 if pin.dtype == torch.float32 else torch.float64
    pdev = pin.reshape((ncol, nt) if hybrid else (ncol, nlev, nt)).to(device=dev, dtype=pdt).contiguous()
    outs = interp_device(src, plev * 100.0, ps=pdev if hybrid else None, p=None if hybrid else pdev, hyam=hyam,
                         hybm=hybm, p0=float(p0), method=method, edge=edge)
    del src, pdev
    if two_d:
        outs = [o.reshape(ncol, plev.size) for o in outs]

    # ---- the kind that came in ----
    res = []
    for x, v, o in zip(fl, vals, outs):
        if not on_device:
            o = o.to(v.device) if isinstance(_values(x), torch.Tensor) else o.cpu().numpy()
        if kind == "raw":
            res.append(o)
            continue
        dims = list(x.dims)
        coords = {k: c for k, c in dict(getattr(x, "coords", {}) or {}).items() if k != dims[1]}
        if kind == "labeled":
            coords = {k: c for k, c in coords.items() if k in dims}
        dims[1] = "plev"
        coords["plev"] = plev
        res.append(containers.make_like("labeled" if on_device else kind, o, tuple(dims), coords,
                                        getattr(x, "name", None), getattr(x, "attrs", None)))
    return (res[0] if single else res), plev


def interp_device(fields, plev_pa, *, ps=None, p=None, hyam=None, hybm=None, p0=1e5, method="log", edge="nan", out=None):
    """One ``temxv_interp`` per eight fields.  ``fields``: contiguous device tensors [ncol][nlev][nt] of one dtype;
    ``ps`` [ncol][nt] or ``p`` [ncol][nlev][nt] on the same device; ``plev_pa`` ascending, in Pa.  Returns new tensors
    [ncol][nplev][nt] (or fills ``out``, contiguous tensors of that shape and dtype); the call is ordered on the
    current stream."""
    import torch
    lib = _vert.load()
    f0 = fields[0]
    ncol, nlev, nt = (int(s) for s in f0.shape)
    plev_pa = np.ascontiguousarray(plev_pa, dtype=np.float64)
    nplev = int(plev_pa.shape[0])
    pin = ps if ps is not None else p
    for t in list(fields) + [pin]:
        if not (t.is_cuda and t.device == f0.device and t.is_contiguous()):
            raise ValueError("interp_device needs contiguous tensors on one device")
    dts = {torch.float64: _vert.F64, torch.float32: _vert.F32}
    dp = C.POINTER(C.c_double)
    with torch.cuda.device(f0.device):
        outs = list(out) if out is not None else [
            torch.empty((ncol, nplev, nt), dtype=f0.dtype, device=f0.device) for _ in fields]
        for o in outs:
            if not (o.is_cuda and o.device == f0.device and o.dtype == f0.dtype and o.is_contiguous()
                    and tuple(o.shape) == (ncol, nplev, nt)) or len(outs) != len(fields):
                raise ValueError("out needs one contiguous %s tensor of shape %s per field" % (f0.dtype, (ncol, nplev, nt)))
        stream = C.c_void_p(torch.cuda.current_stream(f0.device).cuda_stream)
        for g in range(0, len(fields), _vert.NF_MAX):
            fs, os_ = fields[g:g + _vert.NF_MAX], outs[g:g + _vert.NF_MAX]
            sp = (C.c_void_p * len(fs))(*[t.data_ptr() for t in fs])
            op = (C.c_void_p * len(fs))(*[t.data_ptr() for t in os_])
            _vert.check(lib.temxv_interp(
                f0.device.index or 0, len(fs), sp, op, dts[f0.dtype], ncol, nlev, nt, nplev,
                plev_pa.ctypes.data_as(dp), _vert.P_HYBRID if ps is not None else _vert.P_FIELD,
                hyam.ctypes.data_as(dp) if ps is not None else None,
                hybm.ctypes.data_as(dp) if ps is not None else None, float(p0),
                C.c_void_p(pin.data_ptr()), dts[pin.dtype], _vert.METHODS[method], _vert.EDGES[edge], stream))
    return outs


def interp_to_pressure(fields, plev_hpa, *, ps=None, hyam=None, hybm=None, p0=1e5, p=None, method="log", edge="nan",
                       device=None):
    """Interpolate model-level fields to the pressure levels ``plev_hpa`` [hPa] on the GPU.

    ``fields``: one array or a list of arrays laid out ``[ncol][lev][time]`` (or ``[ncol][lev]``), levels top first --
    numpy arrays, torch tensors or labelled arrays (their second dim is the level dim; the result names it ``plev``).
    The result is of the same kind, on the target levels, fp32 when every field is fp32 and fp64 otherwise.
    A descending ``plev_hpa`` is accepted; the result is on ascending levels, like the front end's ``plev``.

    Source pressure, exactly one of
      * ``ps=`` [ncol][time] in Pa with ``hyam=``, ``hybm=`` [lev] and ``p0=``: hybrid levels,
        ``p = hyam * p0 + hybm * ps``, formed in fp64 on the device -- no 3-d pressure array exists;
      * ``p=`` [ncol][lev][time] in Pa: the pressure of every point, for other vertical coordinates.

    ``method``: ``"log"`` linear in ln p (default) or ``"linear"`` linear in p.
    ``edge``: ``"nan"`` -- a target outside the column's first and last level is NaN; ``"hold"`` -- above the top
    level and between the bottom level and the surface the nearest level's value is held, below the surface (in
    ``p=`` mode: below the bottom level) the result is still NaN.  A column whose pressures are not finite and
    strictly increasing comes back NaN; with ``method="log"`` so does one with a pressure <= 0 (interface levels whose
    first pressure is 0 have no ln p), while ``method="linear"`` takes any finite increasing pressures.  NaN below
    ground is what ``TEMDiagnostics(missing="mask")`` takes.

    Raises ``ValueError`` before any device work for inconsistent arguments, shapes, repeated levels, and hybrid
    coefficients that are not monotone over the range of ``ps``.
    """
    return _interp(fields, plev_hpa, ps=ps, hyam=hyam, hybm=hybm, p0=p0, p=p, method=method, edge=edge,
                   device=device)[0]


# ---- time-major model-level records: window -> pressure levels in engine layout ---------------------------------------
def records_to_pressure_device(srcs, ps, plev_pa, *, hyam, hybm, p0=1e5, t0=0, ntb=None, method="log", edge="nan",
                               dtype=None, out=None, path=None):
    """Device tensors ``[nt][nlev][ncol]`` on hybrid levels and ``ps`` ``[nt][ncol]`` -> list of ``[ncol][nplev][ntb]``
    tensors: the snapshots ``t0 .. t0 + ntb`` (default: to the end) on the pressure levels ``plev_pa`` (ascending, Pa),
    in the engine's layout.  The analogue of ``layout.to_engine_layout`` for model-level records.

    ``srcs``: contiguous float64 / float32 tensors of one shape on one device (a single tensor is taken as a list of
    one), levels top first; ``ps`` float64 or float32.  ``dtype``: float32 when every source is float32, float64
    otherwise (float32 widens exactly, float64 is never narrowed).  ``out``: tensors to write into instead of new ones.

    ``path="fused"``: one ``temxi_records_to_pressure`` per eight fields -- each model-level element read once.
    ``path="chain"``: ``to_engine_layout``, a transpose of the ``ps`` window, ``interp_device``.  The two give the same
    bits; ``path=None`` takes the fused call where ``FUSED_RECORDS`` has the work dtype switched on.  The call is
    ordered on the current stream."""
    import torch
    srcs = [srcs] if isinstance(srcs, torch.Tensor) else list(srcs)
    if not srcs:
        raise ValueError("no sources given")
    if path not in (None, "fused", "chain"):
        raise ValueError("path must be None, 'fused' or 'chain', got %r" % (path,))
    if method not in _vert.METHODS:
        raise ValueError("method must be 'log' or 'linear', got %r" % (method,))
    if edge not in _vert.EDGES:
        raise ValueError("edge must be 'nan' or 'hold', got %r" % (edge,))
    s0 = srcs[0]
    dts = {torch.float64: _ingest.F64, torch.float32: _ingest.F32}
    for s in srcs:
        if not (isinstance(s, torch.Tensor) and s.is_cuda and s.device == s0.device):
            raise ValueError("records_to_pressure_device needs device tensors on one device")
        if s.dim() != 3 or tuple(s.shape) != tuple(s0.shape) or not s.is_contiguous():
            raise ValueError("records_to_pressure_device needs contiguous [nt][nlev][ncol] tensors of one shape")
        if s.dtype not in dts:
            raise ValueError("records_to_pressure_device takes float64 and float32, got %s" % s.dtype)
    nt_src, nlev, ncol = (int(n) for n in s0.shape)
    if not (isinstance(ps, torch.Tensor) and ps.is_cuda and ps.device == s0.device and ps.is_contiguous()
            and tuple(ps.shape) == (nt_src, ncol) and ps.dtype in dts):
        raise ValueError("ps must be a contiguous float64 / float32 tensor of shape %s on %s" % ((nt_src, ncol), s0.device))
    t0 = int(t0)
    ntb = nt_src - t0 if ntb is None else int(ntb)
    if t0 < 0 or ntb < 1 or t0 + ntb > nt_src:
        raise ValueError("window t0 = %d, ntb = %d does not lie in 0 .. %d" % (t0, ntb, nt_src))
    if dtype is None:
        dtype = torch.float32 if all(s.dtype == torch.float32 for s in srcs) else torch.float64
    if dtype not in dts:
        raise ValueError("dtype must be float64 or float32, got %s" % (dtype,))
    plev_pa = np.ascontiguousarray(plev_pa, dtype=np.float64)
    hyam = np.ascontiguousarray(hyam, dtype=np.float64).ravel()
    hybm = np.ascontiguousarray(hybm, dtype=np.float64).ravel()
    if plev_pa.ndim != 1 or plev_pa.size < 1 or hyam.shape[0] != nlev or hybm.shape[0] != nlev:
        raise ValueError("plev_pa must be 1-d and hyam / hybm must have %d entries" % nlev)
    nplev = int(plev_pa.shape[0])
    if path is None:
        path = "fused" if FUSED_RECORDS[str(dtype).replace("torch.", "")] else "chain"
    with torch.cuda.device(s0.device):
        if out is None:            # one allocation for all fields
            out = torch.empty((len(srcs), ncol, nplev, ntb), dtype=dtype, device=s0.device).unbind(0)
        out = list(out)
        if len(out) != len(srcs):
            raise ValueError("out has %d tensors for %d sources" % (len(out), len(srcs)))
        for o in out:
            if not (o.is_cuda and o.device == s0.device and o.dtype == dtype and o.is_contiguous()
                    and tuple(o.shape) == (ncol, nplev, ntb)):
                raise ValueError("out needs contiguous %s tensors of shape %s on %s" % (dtype, (ncol, nplev, ntb), s0.device))
        if path == "chain":
            eng = layout.to_engine_layout(srcs, t0, ntb, False, dtype)
            pst = ps[t0:t0 + ntb].t().contiguous()
            interp_device(eng, plev_pa, ps=pst, hyam=hyam, hybm=hybm, p0=float(p0), method=method, edge=edge, out=out)
            return out
        lib = _ingest.load()
        dp = C.POINTER(C.c_double)
        stream = C.c_void_p(torch.cuda.current_stream(s0.device).cuda_stream)
        for g in range(0, len(srcs), _ingest.NF_MAX):
            ss, oo = srcs[g:g + _ingest.NF_MAX], out[g:g + _ingest.NF_MAX]
            sp = (C.c_void_p * len(ss))(*[t.data_ptr() for t in ss])
            sd = (C.c_int * len(ss))(*[dts[t.dtype] for t in ss])
            op = (C.c_void_p * len(ss))(*[t.data_ptr() for t in oo])
            _ingest.check(lib.temxi_records_to_pressure(
                s0.device.index or 0, len(ss), sp, sd, op, dts[dtype], ncol, nlev, nt_src, t0, ntb, nplev,
                plev_pa.ctypes.data_as(dp), hyam.ctypes.data_as(dp), hybm.ctypes.data_as(dp), float(p0),
                C.c_void_p(ps.data_ptr()), dts[ps.dtype], _vert.METHODS[method], _vert.EDGES[edge], stream))
    return out


class _RecordStep:
    """One time block of time-major model-level tensors -> pressure-level engine-layout tensors.  ``tensors`` are the
    fields, then ``ps`` (hybrid levels) or the pressure field ``p_model`` (then the chain serves: the pressure is
    re-laid out like one more field and ``temxv_interp`` runs in field mode)."""

    def __init__(self, nf, plev_pa, hyam, hybm, p0, method, edge, work, field_mode, path):
        self.nf, self.plev_pa, self.hyam, self.hybm, self.p0 = nf, plev_pa, hyam, hybm, float(p0)
        self.method, self.edge, self.work, self.field_mode = method, edge, work, bool(field_mode)
        if field_mode:
            path = "chain"
        elif path is None:
            path = "fused" if FUSED_RECORDS[str(work).replace("torch.", "")] else "chain"
        self.path = path
        self.input_path = "ingest" if path == "fused" else "relayout+interp"

    def __call__(self, tensors, t0, ntb, out):
        srcs, pin = list(tensors[:self.nf]), tensors[self.nf]
        if not self.field_mode:
            return records_to_pressure_device(srcs, pin, self.plev_pa, hyam=self.hyam, hybm=self.hybm, p0=self.p0, t0=t0,
                                              ntb=ntb, method=self.method, edge=self.edge, dtype=self.work, out=out,
                                              path=self.path)
        eng = layout.to_engine_layout(srcs, t0, ntb, False, self.work)
        peng = layout.to_engine_layout([pin], t0, ntb, False, pin.dtype)[0]
        return interp_device(eng, self.plev_pa, p=peng, method=self.method, edge=self.edge, out=out)


class DeviceRecordBlocks:
    """Block source of a TEM run over time-major model-level device tensors: one fused or chained call per block,
    straight from the caller's tensors.  The device holds the source plus one pressure-level block."""

    def __init__(self, tensors, step):
        self.tensors, self.step = list(tensors), step
        self.input_path = step.input_path
        self._out = None
        self.timing = None

    def start(self, blocks):
        self.blocks = list(blocks)

    def get(self, n):
        t0, t1 = self.blocks[n]
        if self._out is not None and self._out[0].shape[2] != t1 - t0:
            self._out = None                      # the short last block: the full one is released first
        self._out = self.step(self.tensors, t0, t1 - t0, self._out)
        return self._out

    def after_launch(self, n):
        pass

    def done(self, n):
        pass

    def close(self):
        self._out = None


class HostRecordBlocks(layout.HostBlocks):
    """Block source of a TEM run over time-major model-level host arrays (``np.ndarray``, ``np.memmap``, CPU tensors):
    the block of every field and of ``ps`` (or of the pressure field) goes up through the two-slot pinned ring of
    ``layout.HostBlocks``; the step on the compute stream is the fused or chained remap instead of the re-layout, and
    ``timing`` reports it as ``ingest_ms``."""

    def __init__(self, arrays, device, step):
        super().__init__(arrays, device, False, step.work, step=lambda slot, ntb, out: step(slot, 0, ntb, out),
                         step_name="ingest_ms")
        self.input_path = step.input_path


def finite_range(ps, rows=4096):
    """(min, max) of the finite values of ``ps`` [nt][...], or None when there are none; a host array is read
    ``rows`` snapshots at a time (a memmap is never loaded whole), a device tensor in one reduction."""
    import torch
    lo, hi = np.inf, -np.inf
    if isinstance(ps, torch.Tensor) and ps.is_cuda:
        fin = torch.isfinite(ps)
        if bool(fin.any()):
            lo = float(torch.where(fin, ps, torch.full_like(ps, float("inf"))).min())
            hi = float(torch.where(fin, ps, torch.full_like(ps, float("-inf"))).max())
    else:
        a = ps.numpy() if isinstance(ps, torch.Tensor) else ps
        for r in range(0, a.shape[0], rows):
            blk = np.asarray(a[r:r + rows])
            blk = blk[np.isfinite(blk)]
            if blk.size:
                lo, hi = min(lo, float(blk.min())), max(hi, float(blk.max()))
    return None if lo > hi else (lo, hi)
