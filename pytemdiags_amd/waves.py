"""Zonal wavenumbers on the native grid (not in the reference): which waves carry the eddy forcing.

``TEMDiagnostics(..., lon=lon_native, wavenumbers=(1, 2, 3))`` fits every requested zonal wavenumber ``m`` to the eddies
of ``ua va theta wap`` on the unstructured grid itself -- a least-squares fit on ``Pbar_l^m(sin lat) cos(m lon)`` and
``... sin(m lon)``, ``l = m..L``, the counterpart of the reference's zonal mean on the ``m = 0`` harmonics; no remap to a
lat-lon grid, no FFT -- and ``tem.waves`` holds

* ``tem.waves[m]``: a result set like ``tem.climatology.stationary`` -- the ten result methods, the sixteen zonal
  attributes and ``results()``, each ``(lat, plev, time)`` -- of a TEM whose eddy fluxes ``upvpb upwappb vptpb`` are the
  wave-``m`` fluxes ``[x'_m y'_m] = (Xc Yc + Xs Ys) / 2``; the mean state is that of the ordinary run.  On each set
  ``parts(name)`` gives ``(Xc, Xs)`` of ``name`` in ``ua va theta wap`` on the zonal grid, ``amplitude(name)``
  ``sqrt(Xc^2 + Xs^2)`` and ``phase(name)`` ``atan2(Xs, Xc) / m``, the longitude of the ridge in radians;
* ``tem.waves.residual``: the same with (total fluxes - sum over the requested m);
* ``tem.waves.wavenumbers`` and ``tem.waves.workspace_bytes``.

``epfy``, ``epfz`` and ``utendepfd`` are linear in the three fluxes: over the requested sets plus ``residual`` they add
up to the ordinary run's (``epdiv`` consumes the already-cast ``epfy`` / ``epfz`` and is additive up to that cast only).
The sum over m alone is NOT the total: noise, and the leakage between m and m +- 4 on a cubed sphere, stay in the
residual.  The numbers come from the HIP engine (pytemdiags_amd/include/temx_wave.h); this module
validates, drives and labels.

``wave_form="classes"`` (default ``"generic"``) runs the same fit in its class form (pytemdiags_amd/include_wavecls/temx_wavecls.h,
DESIGN.md 8c): on a grid whose columns share latitudes -- a cubed sphere, a lat-lon or Gaussian grid -- the sums of the fit
are formed per latitude class and the state keeps a few bytes per column instead of a basis of ``2 (L + 1 - m)`` columns.
It serves ``L + 1 - m <= 64``; a grid without latitude classes and a wider basis are refused with a ``ValueError`` that
names the generic form.  Nothing selects it automatically.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import climatology as clim

FIELD_NAMES = ("ua", "va", "theta", "wap")
WAVE_FORMS = ("generic", "classes")
_FIELD_SRC = {"ua": "ua", "va": "va", "theta": "ta", "wap": "wap"}


def check_wavenumbers(wavenumbers, L):
    """``wavenumbers`` as a tuple of distinct ints in 1..L (ValueError otherwise).  Host logic only."""
    try:
        ms = list(wavenumbers)
    except TypeError:
        ms = [wavenumbers]
    if not ms:
        raise ValueError("wavenumbers is empty: give at least one zonal wavenumber in 1..L")
    out = []
    for m in ms:
        if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)):
            raise ValueError("wavenumbers must be integers in 1..L = %d, got %r" % (L, m))
        if not 1 <= int(m) <= int(L):
            raise ValueError("wavenumber %d is not in 1..L = %d" % (int(m), L))
        if int(m) in out:
            raise ValueError("wavenumber %d is given twice" % int(m))
        out.append(int(m))
    return tuple(out)


def check_lon(lon, ncol):
    """``lon`` (degrees) as a float64 array of ``ncol`` finite values (ValueError otherwise).  Host logic only."""
    if lon is None:
        raise ValueError("wavenumbers= needs lon=: the longitudes of the native columns in degrees")
    v = lon.values if hasattr(lon, "values") and not isinstance(lon, np.ndarray) else lon
    if hasattr(v, "detach"):
        v = v.detach().cpu().numpy()
    v = np.ascontiguousarray(v, dtype=np.float64).ravel()
    if v.size != int(ncol):
        raise ValueError("lon has %d entries but the grid has %d columns" % (v.size, ncol))
    if not np.all(np.isfinite(v)):
        raise ValueError("lon must be finite")
    return v


def check_form(wave_form, have_wavenumbers=True, what="wavenumbers="):
    """``wave_form`` as one of ``WAVE_FORMS`` (ValueError otherwise, and for the class form without ``what``).  Host
    logic only."""
    if not isinstance(wave_form, str) or wave_form not in WAVE_FORMS:
        raise ValueError("wave_form must be one of %s, got %r" % (WAVE_FORMS, wave_form))
    if wave_form == "classes" and not have_wavenumbers:
        raise ValueError("wave_form='classes' needs %s: it is a form of the wave fit" % what)
    return wave_form


def check_arguments(wavenumbers, lon, ncol, L, *, missing="raise", lat_bins=None, time_block=None, climatology=False,
                    wave_form="generic"):
    """Everything ``TEMDiagnostics`` refuses next to ``wavenumbers=`` before any device work -> (tuple of m, lon)."""
    check_form(wave_form)
    ms = check_wavenumbers(wavenumbers, L)
    lon = check_lon(lon, ncol)
    for on, what, why in ((missing == "mask", "missing='mask'", "a masked wave fit"),
                          (bool(lat_bins), "lat_bins", "the latitude-bin form"),
                          (time_block is not None, "time_block=", "a blocked run keeps no native-grid fields"),
                          (bool(climatology), "climatology=True", "wave sets of a time mean")):
        if on:
            raise ValueError("wavenumbers and %s exclude each other (%s is not served yet)" % (what, why))
    return ms, lon


class WaveState:
    """The engine's wave state of some wavenumbers on a finalised plan: the generic form (temxk_wave) or, with
    ``form="classes"``, the class form (temxz_wave), which has the same calls.  It uses the plan: close it first."""

    def __init__(self, plan, lon_deg, wavenumbers, form="generic"):
        self.form = check_form(form)
        if self.form == "classes":
            from . import _wavecls
            self.lib, self._prefix = _wavecls.load(), "temxz_wave_"
        else:
            from . import _wave
            self.lib, self._prefix = _wave.load(), "temxk_wave_"
        self.plan = plan
        self.wavenumbers = tuple(int(m) for m in wavenumbers)
        self._h = C.c_void_p()
        lon = np.ascontiguousarray(lon_deg, dtype=np.float64)
        ms = (C.c_int * len(self.wavenumbers))(*self.wavenumbers)
        try:
            _lib.check(self._fn("create")(C.byref(self._h), plan._h, lon.ctypes.data_as(C.POINTER(C.c_double)),
                                          len(self.wavenumbers), ms))
        except _lib.TemxError as e:
            # what only the class form refuses (a grid without latitude classes, more than 64 degrees) is a choice of
            # the caller's, not a failure of the engine: the way out is the generic form
            if self.form == "classes" and e.code == -6 and "generic form" in str(e):
                raise ValueError("wave_form='classes' does not serve this case: %s" % e) from None
            raise

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    @property
    def workspace_bytes(self):
        return int(self._fn("workspace_bytes")(self._h)) if self._h.value else 0

    def launch(self, m, nf, D):
        """Class form only: how the sweep of ``nf`` (4: the fluxes, 1: a projection) fields of ``D`` columns is cut, as
        ``_wavecls.launch`` gives it."""
        from . import _wavecls
        if self.form != "classes":
            raise ValueError("launch describes the class form: build the state with form='classes'")
        self._live()
        return _wavecls.launch(self._h, self.wavenumbers.index(int(m)), nf, D)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def status(self):
        """Synchronise; True when a non-finite value reached the sums of ``project`` / ``fluxes`` since the last call."""
        self._live()
        f = C.c_int(0)
        _lib.check(self._fn("status")(self._h, C.byref(f), self.plan._stream()))
        return bool(f.value)

    def _live(self):
        if not self._h.value or not self.plan._h.value:
            raise _lib.TemxError(-5, "the wave state or its plan has been closed")

    def project(self, A, m, want_coef=False):
        """``A`` ``[ncol][...]`` on the plan's device -> parts ``[2][M][...]`` (Xc, Xs) fp64, and the coefficients
        ``[Kc][D]`` when asked for."""
        import torch
        from .engine import _DT, _ptr
        self._live()
        plan = self.plan
        A = plan._field(A)
        D = A.numel() // plan.N
        parts = torch.empty((2, plan.M) + tuple(A.shape[1:]), dtype=torch.float64, device=plan.device)
        coef = None
        if want_coef:
            coef = torch.empty((2 * (plan.L + 1 - int(m)), D), dtype=torch.float64, device=plan.device)
        fields = (C.c_void_p * 1)(A.data_ptr())
        dts = (C.c_int * 1)(_DT[A.dtype])
        _lib.check(self._fn("project")(self._h, self.wavenumbers.index(int(m)), 1, fields, dts, D, _ptr(parts),
                                        _ptr(coef) if coef is not None else None, plan._stream()))
        return (parts, coef) if want_coef else parts

    def fluxes(self, ua, va, ta, wap, want_parts=False):
        """-> flux ``[nm][3][M][nlev][nt]`` (u'v', u'omega', v'theta' of every wavenumber) and parts
        ``[nm][4][2][M][nlev][nt]`` (Xc, Xs of ua va theta wap) or None.  Needs ``plan.set_tem``."""
        import torch
        from .engine import _ptr
        self._live()
        plan = self.plan
        (u, v, t, w), dt = plan._four(ua, va, ta, wap)
        nm = len(self.wavenumbers)
        flux = torch.empty((nm, 3, plan.M, plan.nlev, plan.nt), dtype=torch.float64, device=plan.device)
        parts = None
        if want_parts:
            parts = torch.empty((nm, 4, 2, plan.M, plan.nlev, plan.nt), dtype=torch.float64, device=plan.device)
        _lib.check(self._fn("fluxes")(self._h, _ptr(u), _ptr(v), _ptr(t), _ptr(w), dt, _ptr(flux),
                                       _ptr(parts) if parts is not None else None, plan._stream()))
        return flux, parts


class WaveSet(clim.ResultSet):
    """``tem.waves[m]`` (and ``tem.waves.residual``, which has no parts): the result set of ``climatology.ResultSet``
    whose eddy fluxes are those of one zonal wavenumber, plus the wave-m components of the fields on the zonal grid."""

    def __init__(self, owner, name, res, zon, m=None, parts=None):
        super().__init__(owner, name, res, zon, None)
        self.m, self._parts = m, parts

    def _pair(self, name):
        if self._parts is None:
            raise RuntimeError("the residual set has no wave components: ask tem.waves[m]")
        if name not in FIELD_NAMES:
            raise ValueError("name must be one of %s, got %r" % (FIELD_NAMES, name))
        p = self._parts[FIELD_NAMES.index(name)]
        return p[0], p[1]

    def _label(self, t, name, what):
        return self._owner._wrap(t, "%s_%s_m%d" % (name, what, self.m), _FIELD_SRC[name], force64=name == "theta")

    def parts(self, name):
        """(cos part Xc, sin part Xs) of the wave-m component of ``name``: ``x'_m = Xc cos(m lon) + Xs sin(m lon)``."""
        xc, xs = self._pair(name)
        return self._label(xc, name, "cos"), self._label(xs, name, "sin")

    def amplitude(self, name):
        import torch
        xc, xs = self._pair(name)
        return self._label(torch.sqrt(xc * xc + xs * xs), name, "amplitude")

    def phase(self, name):
        """Longitude of the ridge of the wave-m component, ``atan2(Xs, Xc) / m`` in radians."""
        import torch
        xc, xs = self._pair(name)
        return self._label(torch.atan2(xs, xc) / float(self.m), name, "phase")


class TEMWaves:
    """``tem.waves``: ``wavenumbers``, ``tem.waves[m]``, ``residual``, ``workspace_bytes`` (device bytes the engine's
    wave state held: the stored bases, ncol x Kc x 8 bytes per wavenumber, and the workspace of the run)."""

    def __init__(self, wavenumbers, sets, residual, workspace_bytes, form="generic"):
        self.wavenumbers = tuple(wavenumbers)
        self.residual = residual
        self.workspace_bytes = int(workspace_bytes)
        self.form = form                          # "generic" or "classes": the form of the fit that made the sets
        self._sets = dict(zip(self.wavenumbers, sets))

    def __getitem__(self, m):
        try:
            return self._sets[int(m)]
        except (KeyError, TypeError, ValueError):
            raise KeyError("wavenumber %r was not requested (wavenumbers = %s)" % (m, self.wavenumbers)) from None

    def __iter__(self):
        return iter(self.wavenumbers)

    def __len__(self):
        return len(self.wavenumbers)


def build(owner, plan, lon, wavenumbers, fields, zon, form="generic"):
    """The wave sets of a finished ordinary run: ``plan`` still set for its (nlev, nt), ``fields`` the four device
    fields, ``zon`` its sixteen zonal intermediates (whose seven zonal means the sets share).  -> TEMWaves."""
    state = WaveState(plan, lon, wavenumbers, form=form)
    try:
        flux, parts = state.fluxes(*fields, want_parts=True)      # (the ordinary run has refused non-finite fields)
        nbytes = state.workspace_bytes
    finally:
        state.close()
    i0 = _lib.ZONAL_NAMES.index(clim.FLUX_NAMES[0])
    sets = []
    zm7 = zon[:7].clone()
    for i, m in enumerate(wavenumbers):
        zm7[i0:i0 + 3] = flux[i]
        res, z = plan.tem_from_zonal_means(zm7, want_zonal=True)
        sets.append(WaveSet(owner, "wave%d" % m, res, z, m=m, parts=parts[i]))
    zm7[i0:i0 + 3] = zon[i0:i0 + 3] - flux.sum(dim=0)
    res, z = plan.tem_from_zonal_means(zm7, want_zonal=True)
    return TEMWaves(wavenumbers, sets, WaveSet(owner, "residual", res, z), nbytes, form)
