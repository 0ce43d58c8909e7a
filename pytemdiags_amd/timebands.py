"""EP flux by time scale (not in the reference): which band of frequencies carries the eddy forcing.

``TEMDiagnostics(..., time_bands={"synoptic": w_a, "low": w_b})`` filters ``ua va ta wap`` along time with every band's
weights (a centred finite-impulse-response filter, ``x_b[t] = sum_k w[k + h] x[t + k]``, ``k = -h..h``), runs the plan's
TEM on each filtered record and keeps its three eddy fluxes ``upvpb upwappb vptpb``; ``tem.bands`` then holds

* ``tem.bands[name]``: a result set like ``tem.climatology.stationary`` -- the ten result methods, the sixteen zonal
  attributes and ``results()`` -- at ``(lat, plev, NT - 2h)`` with the time coordinate ``time[h:NT - h]``: the unchanged
  epilogue of a TEM run on the ORDINARY run's mean state ``ub vb thetab wapb`` at those times and the band's fluxes.  A
  TEM of band-passed fields alone is meaningless -- their zonal mean is near zero, so psi divides by a d(thetab)/dp near
  zero -- which is why the combination lives here and not in the caller's hands;
* ``tem.bands.residual``: the same with (total fluxes - sum over the bands); the cross-band terms live there;
* ``tem.bands.time_mean()``: the same sets at ``(lat, plev, 1)``, from the time means over the valid times of the seven
  zonal means (``epfy`` of the mean, not the mean of ``epfy``);
* ``names``, ``half_width``, ``weights`` (``[nb][2h + 1]``, padded), ``filter_path`` (``"kernel"``) and
  ``workspace_bytes`` (device bytes of the filtered copies and the weight table).

Bands of unequal length are zero-padded, centred, to the longest, so all share the half-width ``h`` and the valid times.
``epfy``, ``epfz`` and ``utendepfd`` are linear in the three fluxes: over the bands plus ``residual`` they add up to the
ordinary run's at ``[h:NT - h]``.  ``lanczos`` gives Duchon's weights.  The filter is the HIP kernel of
pytemdiags_amd/include/temx_tfilt.h (one call for the four fields and all bands: the record is read once); this module
validates, drives and labels.  Not served: ``time_block=`` (a block needs a halo of the next one), ``missing="mask"`` (a
missing value poisons its window), and a band split next to ``climatology=True`` or ``wavenumbers=``.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from . import climatology as clim

NB_MAX = 4
NW_MIN, NW_MAX = 3, 255


def lanczos(nweights, low=None, high=None):
    """Duchon's (1979) Lanczos weights, float64 ``[nweights]``, ``nweights`` odd in 3..255; cutoffs in cycles per time
    step, in (0, 0.5).

    ``low=fc`` alone: the low-pass that keeps frequencies below ``fc``,
    ``w_k = sin(2 pi fc k) / (pi k) * sin(pi k / n) / (pi k / n)``, ``w_0 = 2 fc``, ``n = (nweights - 1) / 2``, scaled
    to sum 1.  ``high=fc`` alone: the high-pass that keeps frequencies above ``fc``, the unit impulse minus that
    low-pass (sum 0).  Both: the band-pass that keeps ``high < f < low``, the low-pass at ``low`` minus the low-pass
    at ``high`` (sum 0); it needs ``high < low``.  Host numpy."""
    if isinstance(nweights, (bool, np.bool_)) or not isinstance(nweights, (int, np.integer)):
        raise ValueError("nweights must be an odd integer in %d..%d, got %r" % (NW_MIN, NW_MAX, nweights))
    nw = int(nweights)
    if nw % 2 == 0 or not NW_MIN <= nw <= NW_MAX:
        raise ValueError("nweights must be an odd integer in %d..%d, got %r" % (NW_MIN, NW_MAX, nweights))
    if low is None and high is None:
        raise ValueError("lanczos needs low= (low-pass), high= (high-pass) or both (band-pass)")
    for name, fc in (("low", low), ("high", high)):
        if fc is not None and not 0.0 < float(fc) < 0.5:
            raise ValueError("%s must lie in (0, 0.5) cycles per time step, got %r" % (name, fc))
    if low is not None and high is not None and not float(high) < float(low):
        raise ValueError("a band-pass keeps high < f < low: high = %r is not below low = %r" % (high, low))
    n = (nw - 1) // 2

    def lowpass(fc):
        k = np.arange(1, n + 1, dtype=np.float64)
        half = np.sin(2.0 * np.pi * fc * k) / (np.pi * k) * (np.sin(np.pi * k / n) / (np.pi * k / n))
        w = np.concatenate([half[::-1], [2.0 * fc], half])
        w /= math.fsum(w)
        w[n] -= math.fsum(w) - 1.0          # the sum is 1 to the last bit the centre weight can give
        return w

    if high is None:
        return lowpass(float(low))
    w = -lowpass(float(high))
    if low is None:
        w[n] += 1.0
    else:
        w += lowpass(float(low))
    w[n] -= math.fsum(w)
    return w


def check_bands(time_bands):
    """``time_bands`` -> (names, weights ``[nb][2h + 1]`` float64 zero-padded and centred, h).  ValueError for anything
    but a mapping of 1..4 non-empty string names to 1-D sequences of finite weights of odd length in 3..255.  Host
    logic only."""
    if not hasattr(time_bands, "items") or not hasattr(time_bands, "keys"):
        raise ValueError("time_bands must be a mapping of band names to filter weights, got %r" % type(time_bands).__name__)
    if not 1 <= len(time_bands) <= NB_MAX:
        raise ValueError("time_bands must hold 1..%d bands, got %d" % (NB_MAX, len(time_bands)))
    names, ws = [], []
    for name, w in time_bands.items():
        if not isinstance(name, str) or not name:
            raise ValueError("time_bands: band names must be non-empty strings, got %r" % (name,))
        if hasattr(w, "detach"):
            w = w.detach().cpu().numpy()
        try:
            a = np.asarray(w, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("time_bands[%r]: the weights must be a one-dimensional sequence of numbers" % name) from None
        if a.ndim != 1:
            raise ValueError("time_bands[%r]: the weights must be a one-dimensional sequence, got %d dims" % (name, a.ndim))
        if a.size % 2 == 0 or not NW_MIN <= a.size <= NW_MAX:
            raise ValueError("time_bands[%r]: the number of weights must be odd and in %d..%d, got %d"
                             % (name, NW_MIN, NW_MAX, a.size))
        if not np.all(np.isfinite(a)):
            raise ValueError("time_bands[%r]: the weights must be finite" % name)
        names.append(name)
        ws.append(a)
    nw = max(a.size for a in ws)
    table = np.zeros((len(ws), nw), dtype=np.float64)
    for b, a in enumerate(ws):
        off = (nw - a.size) // 2
        table[b, off:off + a.size] = a
    return tuple(names), table, (nw - 1) // 2


def check_arguments(time_bands, *, missing="raise", time_block=None, climatology=False, wavenumbers=None):
    """Everything ``TEMDiagnostics`` refuses next to ``time_bands=`` before it knows the record's length ->
    (names, weights, h)."""
    out = check_bands(time_bands)
    for on, what, why in ((time_block is not None, "time_block=", "a block needs a halo of the next one, which"),
                          (missing == "mask", "missing='mask'", "a missing value poisons its window: a masked filter"),
                          (bool(climatology), "climatology=True", "the band split of the transient part of a climatology"),
                          (wavenumbers is not None, "wavenumbers=", "band x wavenumber")):
        if on:
            raise ValueError("time_bands and %s exclude each other (%s is not served yet)" % (what, why))
    return out


def check_record(args, nt):
    """The record against the filter: ``NT >= 2h + 1`` (ValueError otherwise).  Host logic only."""
    h = args[2]
    if int(nt) < 2 * h + 1:
        raise ValueError("time_bands: the record has %d times but the filter needs NT >= 2h + 1 = %d" % (int(nt), 2 * h + 1))
    return args


def filter_time(fields, weights, out_dtype=None):
    """``temxf_filter_time`` on up to eight contiguous device tensors ``[ncol][nlev][nt]`` (fp64 or fp32 each) with the
    weight table ``[nb][nw]`` (host or device, float64) -> list of ``nb`` lists of tensors ``[ncol][nlev][nt - nw + 1]``
    of ``out_dtype`` (default: float32 when every field is, else float64), on the current stream."""
    import torch
    from . import _tfilt
    from .engine import _DT
    lib = _tfilt.load()
    fields = [x.contiguous() for x in fields]
    dev = fields[0].device
    shape = tuple(fields[0].shape)
    if len(shape) != 3 or any(tuple(x.shape) != shape or x.device != dev or x.dtype not in _DT for x in fields):
        raise ValueError("fields must be float64 / float32 tensors [ncol][nlev][nt] of one shape on one device")
    if out_dtype is None:
        out_dtype = torch.float32 if all(x.dtype == torch.float32 for x in fields) else torch.float64
    w = torch.as_tensor(np.asarray(weights, dtype=np.float64) if not isinstance(weights, torch.Tensor) else weights)
    w = w.to(device=dev, dtype=torch.float64).contiguous()
    if w.dim() != 2:
        raise ValueError("weights must be [nb][nw]")
    nb, nw = (int(n) for n in w.shape)
    ncol, nlev, nt = shape
    nf = len(fields)
    outs = [[torch.empty((ncol, nlev, max(nt - nw + 1, 0)), dtype=out_dtype, device=dev) for _ in range(nf)] for _ in range(nb)]
    src = (C.c_void_p * nf)(*[x.data_ptr() for x in fields])
    dts = (C.c_int * nf)(*[_DT[x.dtype] for x in fields])
    dst = (C.c_void_p * (nb * nf))(*[o.data_ptr() for band in outs for o in band])
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)    # (the table dies on this stream, behind the kernel)
    _lib.check(lib.temxf_filter_time(dev.index or 0, nf, src, dts, nb, dst, _DT[out_dtype], ncol, nlev, nt, nw,
                                     C.c_void_p(w.data_ptr()), 0, st))
    return outs


class TEMBands:
    """``tem.bands``: ``names``, ``tem.bands[name]``, ``residual``, ``time_mean()``, ``half_width``, ``weights``,
    ``filter_path`` and ``workspace_bytes`` (module docstring)."""

    def __init__(self, owner, plan, names, weights, h, time, zm7, fluxes, workspace_bytes, mean=False):
        self.names = tuple(names)
        self.half_width = int(h)
        self.weights = np.array(weights, dtype=np.float64)
        self.filter_path = "kernel"
        self.workspace_bytes = int(workspace_bytes)
        self.time = time
        self._owner, self._plan, self._zm7, self._fluxes, self._is_mean = owner, plan, zm7, fluxes, mean
        self._mean = None
        i0 = _lib.ZONAL_NAMES.index(clim.FLUX_NAMES[0])
        self._sets = {}
        work = zm7.clone()
        total = zm7[i0:i0 + 3]
        for name, flux in list(zip(self.names, fluxes)) + [("residual", total - sum(fluxes))]:
            work[i0:i0 + 3] = flux
            res, zon = plan.tem_from_zonal_means(work, want_zonal=True)
            self._sets[name] = clim.ResultSet(owner, name, res, zon, time)
        self.residual = self._sets.pop("residual")

    def __getitem__(self, name):
        try:
            return self._sets[name]
        except (KeyError, TypeError):
            raise KeyError("band %r was not requested (time_bands = %s)" % (name, self.names)) from None

    def __iter__(self):
        return iter(self.names)

    def __len__(self):
        return len(self.names)

    def time_mean(self):
        """The same sets at ``(lat, plev, 1)``: the epilogue on the time means, over the valid times, of the mean state
        and of every set's fluxes.  The time coordinate is the mean of the valid times."""
        if self._is_mean:
            return self
        if self._mean is None:
            self._mean = TEMBands(self._owner, self._plan, self.names, self.weights, self.half_width,
                                  clim.mean_time(self.time), self._zm7.mean(dim=-1, keepdim=True),
                                  [f.mean(dim=-1, keepdim=True) for f in self._fluxes], self.workspace_bytes, mean=True)
        return self._mean


class Builder:
    """The device side, driven by ``TEMDiagnostics``: ``run`` on the four resident fields ahead of the ordinary run,
    ``finish`` with the zonal intermediates of the ordinary run."""

    def __init__(self, owner, plan, args):
        self.owner, self.plan = owner, plan
        self.names, self.weights, self.h = args
        self.fluxes = None
        self.workspace_bytes = 0

    def run(self, fields):
        """One filter call for the four fields and every band, then the plan's TEM on each band's record: the plan is
        left set for ``NT - 2h`` times."""
        o, plan = self.owner, self.plan
        fields = list(fields)
        bands = filter_time(fields, self.weights, out_dtype=o._work_dtype)
        self.workspace_bytes = sum(x.numel() * x.element_size() for band in bands for x in band) + self.weights.size * 8
        ntv = int(fields[0].shape[-1]) - 2 * self.h
        plan.set_tem(o.NLEV, ntv, o._p_np, float(o.p0))
        i0 = _lib.ZONAL_NAMES.index(clim.FLUX_NAMES[0])
        self.fluxes = []
        while bands:
            band = bands.pop(0)
            # (the results on the filtered mean state are dropped: a band-pass leaves d(thetab)/dp near zero there)
            _, zon = plan.tem_run(*band, want_zonal=True)
            if plan.status():
                raise RuntimeError(clim._NAN_MESSAGE)
            self.fluxes.append(zon[i0:i0 + 3].clone())
            del band, zon                      # the filtered copies go band by band

    def finish(self, zon_all):
        """``zon_all``: ``[16][M][nlev][NT]`` of the ordinary run, the plan still set for it -> TEMBands."""
        o, h = self.owner, self.h
        nt = int(zon_all.shape[-1])
        zm7 = zon_all[:7, :, :, h:nt - h].contiguous()
        return TEMBands(o, self.plan, self.names, self.weights, h, np.asarray(o.time)[h:nt - h], zm7, self.fluxes,
                        self.workspace_bytes)
