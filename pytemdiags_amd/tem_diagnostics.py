"""Drop-in front end for ``PyTEMDiags.TEMDiagnostics`` (reference: PyTEMDiags/tem_diagnostics.py).

Same constructor, methods, properties and error behaviour.  All numerics -- potential
temperature, the 7 + 4 zonal means, eddy products, p / lat derivatives, psi, the cumulative
pressure integral and the ten GM16 Table-A1 diagnostics -- run on the MI355X in the HIP engine
(libtemx.so); this module only validates, reshapes and labels.

Input kinds (the output kind follows the input kind):
  * labelled arrays -- ``xarray.DataArray`` when xarray is importable, or anything with
    ``.dims`` / ``.values`` and a ``plev`` coordinate (``containers.LabeledArray``);
  * raw ``numpy.ndarray`` / ``torch.Tensor`` laid out as ``dims`` (default
    ``(ncol, plev, time)``) with explicit ``plev=`` [hPa] and optional ``time=``.
"""
from __future__ import annotations

import os
import threading
import warnings

import numpy as np

from . import _lib, containers, layout
from . import climatology as clim
from . import timebands as tb
from . import waves as wv
from .constants import P0, Om
from .sph_zonal_mean import sph_zonal_averager

DEFAULT_DIMS = {"horz": "ncol", "vert": "plev", "time": "time"}        # tem_diagnostics.py:25

# dtype each stored quantity has in the reference when the inputs are not fp64:
# theta is promoted to fp64 by the fp64 pressure einsum (tem_diagnostics.py:498); everything
# downstream of theta, of cos(lat) products or of p_integral is fp64; the rest keeps the input dtype.
# from_model_levels hands a block source (vertical.DeviceRecordBlocks / HostRecordBlocks) to the constructor it calls,
# on the calling thread; the constructor's public signature stays as the reference has it
_pending = threading.local()

_F64_ALWAYS = {"thetab", "vptpb", "dthetab_dp", "ubcoslat", "dubcoslat_dlat", "psi", "psicoslat",
               "dpsicoslat_dlat", "dpsi_dp", "int_vbdp", "thetap", "vptp", "theta"}


class TEMDiagnostics:
    def __init__(self, ua, va, ta, wap, lat_native, q=None, p0=P0, zm_dlat=1, L=50,
                 dim_names=DEFAULT_DIMS, grid_name=None, zm_grid_name=None, map_save_dest=None,
                 overwrite_map=False, zm_pole_points=False, debug_level=1, logfile=None,
                 *, plev=None, time=None, dims=None, device=None, missing="raise", min_coverage=0.5, time_block=None,
                 lat_bins=None, climatology=False, tracer_mask=None, min_time_coverage=None, time_groups=None,
                 time_weights=None, min_group_coverage=None, lon=None, wavenumbers=None, time_bands=None,
                 wave_form="generic"):
        # ---- zonal wavenumbers (not in the reference; waves.py): checked before anything touches the device ----
        self._waves, self._wave_args = None, None
        self._wave_form = wv.check_form(wave_form, wavenumbers is not None)
        if wavenumbers is not None:
            self._wave_args = wv.check_arguments(wavenumbers, lon, len(lat_native), L, missing=missing, lat_bins=lat_bins,
                                                 time_block=time_block, climatology=climatology, wave_form=wave_form)
        # ---- EP flux by time scale (not in the reference; timebands.py): checked before anything touches the device ----
        # (the record's length is checked in _config_dims, still before the device)
        self._bands, self._band_args = None, None
        if time_bands is not None:
            self._band_args = tb.check_arguments(time_bands, missing=missing, time_block=time_block, climatology=climatology,
                                                 wavenumbers=wavenumbers)
        # ---- time-mean TEM (not in the reference; climatology.py): checked before anything touches the device ----
        self.min_group_coverage = clim.check_group_coverage(min_group_coverage, climatology, missing, time_groups,
                                                            time_weights, min_time_coverage)
        self._want_climatology = clim.check_flag(climatology, missing, min_time_coverage, self.min_group_coverage)
        self.min_time_coverage = None if min_time_coverage is None else clim.time_coverage_value(min_time_coverage)
        self._climatology = None
        # (grouped and weighted means: the sizes are checked in _config_dims, still before the device)
        self._group_args = clim.check_group_flags(time_groups, time_weights, climatology, missing, self.min_group_coverage)
        self._groups = None
        # ---- blocked run over the time axis (not in the reference): checked before anything touches the device ----
        self.time_block = layout.check_time_block(time_block)
        self._given_source = getattr(_pending, "source", None)
        _pending.source = None
        # ---- missing-value mode (not in the reference): checked before anything touches the device ----
        if missing not in ("raise", "mask"):
            raise ValueError("missing must be 'raise' or 'mask', got %r" % (missing,))
        if not 0.0 <= float(min_coverage) <= 1.0:
            raise ValueError("min_coverage must lie in [0, 1], got %r" % (min_coverage,))
        self.tracer_mask = self._check_tracer_mask(tracer_mask, missing, q)
        self.missing = missing
        self.min_coverage = float(min_coverage)
        # ---- latitude-bin form (not in the reference; opt-in, include/temx.h): checked before anything touches the device
        self._check_lat_bins(lat_bins, missing)
        # ---- arguments (tem_diagnostics.py:217-236) ----
        self.p0 = p0
        self.q = q
        self.ntrac = None
        self.lat_native = lat_native
        self.L = L
        self.zm_dlat = zm_dlat
        self.dim_names = dim_names
        self.zm_pole_points = zm_pole_points
        self.grid_name = grid_name
        self.zm_grid_name = zm_grid_name
        self.map_save_dest = map_save_dest
        self.overwrite_map = overwrite_map
        self.debug_level = debug_level
        self.logfile = logfile
        self._device = 0 if device is None else device
        self._raw_dims = dims
        self._raw_plev, self._raw_time = plev, time
        self._in = {"ua": ua, "va": va, "ta": ta, "wap": wap}

        self._config_dims()

        # ---- zonal averaging object (tem_diagnostics.py:243-249) ----
        self.ZM = sph_zonal_averager(self._lat_native_np, self._lat_zm, self.L, grid_name=grid_name,
                                     grid_out_name=zm_grid_name, save_dest=map_save_dest,
                                     debug=debug_level > 1, overwrite=overwrite_map, device=self._device,
                                     fp32_fields=str(self._work_dtype) == "torch.float32",
                                     missing=missing, min_coverage=self.min_coverage, lat_bins=lat_bins)
        if self.ZM.Y0 is None or self.ZM.Y0p is None:
            self.ZM.sph_compute_matrices(overwrite=overwrite_map)
        self._zonal_mean = self.ZM.sph_zonal_mean

        # ---- the whole numeric pipeline: one engine call (tem_diagnostics.py:252-259), or one per time block ----
        plan = self.ZM._plan
        self._eddy = None
        self._theta = None
        self._out_file = None
        self._teddy = [None] * self.ntrac
        self._last_tracer = None
        self._after_launch = None
        self.block_timing = None
        self._clim = None
        if self._want_climatology:
            if self._groups is not None and self.min_group_coverage is not None:
                self._clim = clim.MaskedGroupedBuilder(self, plan, self._groups, self.min_group_coverage)
            elif self._groups is not None:
                self._clim = clim.GroupedBuilder(self, plan, self._groups)
            else:
                self._clim = (clim.Builder(self, plan) if self.min_time_coverage is None
                              else clim.MaskedBuilder(self, plan, self.min_time_coverage))
        self._band_builder = None if self._band_args is None else tb.Builder(self, plan, self._band_args)
        if self.time_block is None and self._block_source is None:
            if self._clim is not None:      # time means and their TEM first: the ordinary run is the plan's last
                self._clim.add(self._dev_fields)
                self._clim.run_stationary()
            if self._band_builder is not None:      # the band runs first too, for the same reason
                self._band_builder.run(self._dev_fields)
            plan.set_tem(self.NLEV, self.NT, self._p_np, float(self.p0))
            self._res, self._zon, self._cov, self._tres, self._tzon, self._tcov = self._run_block(
                plan, self._dev_fields, self._dev_q, self.NT)
        else:
            self._run_blocked(plan)
        if self._clim is not None:
            self._climatology = self._clim.finish(self._zon)
            self._clim = None
        if self._band_builder is not None:  # the plan is still set for the ordinary run, whose mean state the sets share
            self._bands = self._band_builder.finish(self._zon)
            self._band_builder = None
        if self._wave_args is not None:     # the plan is still set for the ordinary run, whose zonal means the sets share
            self._waves = wv.build(self, plan, self._wave_args[1], self._wave_args[0], self._dev_fields, self._zon,
                                   form=self._wave_form)

    @property
    def waves(self):
        """``wavenumbers=(m, ...)`` with ``lon=``: the wave-m result sets, ``waves.TEMWaves`` (``tem.waves[m]``,
        ``tem.waves.residual``, ``tem.waves.wavenumbers``, ``tem.waves.workspace_bytes``)."""
        if self._waves is None:
            raise RuntimeError("waves is not available: build the object with lon= and wavenumbers=")
        return self._waves

    @property
    def bands(self):
        """``time_bands={name: weights, ...}``: the result sets by time scale, ``timebands.TEMBands`` (``tem.bands[name]``,
        ``tem.bands.residual``, ``tem.bands.time_mean()``, ``names``, ``half_width``, ``weights``, ``filter_path``,
        ``workspace_bytes``)."""
        if self._bands is None:
            raise RuntimeError("bands is not available: build the object with time_bands=")
        return self._bands

    @property
    def climatology(self):
        """``climatology=True``: the time-mean TEM of the record with its stationary and transient parts, a
        ``climatology.TEMClimatology`` (attributes ``total``, ``stationary``, ``transient``)."""
        if self._climatology is None:
            raise RuntimeError("climatology is not available: build the object with climatology=True")
        return self._climatology

    @staticmethod
    def _check_lat_bins(lat_bins, missing):
        """The TEMX_OPT_LAT_BINS value of ``lat_bins`` (ValueError for a bad one, or next to ``missing="mask"``)."""
        from . import engine
        value = engine.lat_bins_value(lat_bins)
        if value and missing == "mask":
            raise ValueError("lat_bins and missing='mask' exclude each other: the latitude-bin form does not serve "
                             "masked fields")
        return value

    @property
    def lat_bins(self):
        """Number of latitude bins the run used (512 for ``lat_bins=True``), 0 when the latitude-bin form is off."""
        return self.ZM._plan.lat_bins

    @property
    def sweep_form(self):
        """The form of the sweeps this object ran: "binned" (``lat_bins=``), "masked" (``missing="mask"``),
        "single-sweep", "class-sums" or "two-pass"."""
        return self.ZM._plan.sweep_form

    def _run_block(self, plan, fields, qs, nt):
        """One engine run over ``nt`` snapshots in engine layout (``plan.set_tem`` has been called for them):
        the whole record in the default mode, one time block under ``time_block=``.
        -> (results, zonal intermediates, coverage or None, tracer results, tracer zonal intermediates, tracer
        coverages -- empty unless ``tracer_mask="own"``)."""
        # (class-sum forms: the first tracer, when there is one, shares the sweep of the fields, temx_tem_tracer_run;
        #  single sweep: the tracers follow the TEM run in pairs, temx_tracers_run)
        fused = None
        masked_q = self.ntrac and self.missing == "mask"     # tracer_mask="own": one masked run per tracer
        if self.ntrac and not masked_q and not plan.single_sweep:
            res, zon, *fused = plan.tem_tracer_run(*fields, qs[0], want_zonal=True)
        else:
            res, zon = plan.tem_run(*fields, want_zonal=True)
        if self._after_launch is not None:                  # blocked run: the next block goes up behind this one
            self._after_launch()
        # missing="mask": coverage of this run on the zonal grid (the averager's later calls reuse the plan)
        cov = plan.coverage().reshape(self.ZM_N, self.NLEV, nt) if self.missing == "mask" else None
        if plan.status():                                   # sph_zonal_mean.py:219-221
            raise RuntimeError("Variable has nans! Spectral zonal averager cannot handle nans; "
                               "please replace or remove them")
        # ---- tracers (tem_diagnostics.py:532-538, 560-570, 602-611): one engine call each ----
        tres_all, tzon_all, tcov_all = [], [], []
        if masked_q:
            for i in range(self.ntrac):
                tres, tzon, tcov = plan.tracer_run_masked(qs[i], fields[1], fields[3], want_zonal=True)
                tres_all.append(tres)
                tzon_all.append(tzon)
                tcov_all.append(tcov)
                self._last_tracer = i
        elif self.ntrac and plan.single_sweep:
            # the list of tracers in one engine call: two per sweep, (q1, q2, v, omega) read once
            for tres, tzon in plan.tracers_run(qs, fields[1], fields[3], want_zonal=True):
                tres_all.append(tres)
                tzon_all.append(tzon)
            self._last_tracer = self.ntrac - 1
        else:
            for i in range(self.ntrac):
                if i == 0 and fused is not None:
                    tres, tzon = fused
                else:
                    tres, tzon = plan.tracer_run(qs[i], fields[1], fields[3], want_zonal=True)
                tres_all.append(tres)
                tzon_all.append(tzon)
                self._last_tracer = i
        if self.ntrac and plan.status():
            raise RuntimeError("Variable has nans! Spectral zonal averager cannot handle nans; "
                               "please replace or remove them")
        return res, zon, cov, tres_all, tzon_all, tcov_all

    def _run_blocked(self, plan):
        """``time_block=``: every TEM step is independent per snapshot (the tail couples latitude and pressure only),
        so the record runs in the blocks of ``layout.time_blocks`` and the results are gathered on the zonal grid at
        ``[..., t0:t1]``.  The native-grid fields are not kept."""
        import torch
        # (a whole run fed by a block source -- time-major model levels -- is one block, and keeps its fields)
        blocks = layout.time_blocks(self.NT, self.NT if self.time_block is None else self.time_block)
        src = self._block_source
        src.start(blocks)
        big = None
        cur = None
        try:
            for n, (t0, t1) in enumerate(blocks):
                ntb = t1 - t0
                fs = src.get(n)
                if self._clim is not None:
                    # the time sum of the block, on the stream of its TEM run and before the source has it back
                    self._clim.add(fs[:4])
                    if self.time_block is None:
                        # one block whose fields are kept: as in a whole run, the ordinary run is the plan's last
                        self._clim.run_stationary()
                        cur = None
                if self._band_builder is not None:      # (one block whose fields are kept: time_block= is refused)
                    self._band_builder.run(fs[:4])
                    cur = None
                if ntb != cur:
                    plan.set_tem(self.NLEV, ntb, self._p_np, float(self.p0))
                    cur = ntb
                self._after_launch = lambda n=n: src.after_launch(n)
                out = self._run_block(plan, fs[:4], fs[4:], ntb)
                src.done(n)
                if self.time_block is None:
                    self._dev_fields, self._dev_q = list(fs[:4]), list(fs[4:])
                del fs
                if len(blocks) == 1:
                    big = out
                    break
                if big is None:
                    def whole(x):
                        return torch.empty(tuple(x.shape[:-1]) + (self.NT,), dtype=x.dtype, device=x.device)
                    big = (whole(out[0]), whole(out[1]), None if out[2] is None else whole(out[2]),
                           [whole(x) for x in out[3]], [whole(x) for x in out[4]], [whole(x) for x in out[5]])
                big[0][..., t0:t1] = out[0]
                big[1][..., t0:t1] = out[1]
                if out[2] is not None:
                    big[2][..., t0:t1] = out[2]
                for dst, x in zip(big[3] + big[4] + big[5], out[3] + out[4] + out[5]):
                    dst[..., t0:t1] = x
                del out
        finally:
            self._after_launch = None
            src.close()
            self.block_timing = src.timing
            self._block_source = None
        if self._clim is not None and self.time_block is not None:
            self._clim.run_stationary()     # after the last block: a blocked run serves no native outputs
        self._res, self._zon, self._cov, self._tres, self._tzon, self._tcov = big
        self._last_tracer = None

    def _refuse_native(self, what):
        if self.time_block is not None:
            raise RuntimeError("%s is not available with time_block=%d: a blocked run keeps no native-grid fields; "
                               "run without time_block for native outputs" % (what, self.time_block))

    def _input_field(self, i, name):
        self._refuse_native(name)
        return self._dev_fields[i]

    # the inputs on the device, [ncol][plev][time] in the work dtype (a whole run keeps them, a blocked run does not)
    ua = property(lambda s: s._input_field(0, "ua"))
    va = property(lambda s: s._input_field(1, "va"))
    ta = property(lambda s: s._input_field(2, "ta"))
    wap = property(lambda s: s._input_field(3, "wap"))

    @property
    def input_path(self):
        """How the inputs reached the engine's layout: ``"relayout"`` (time-major input, the GPU re-layout of
        ``layout.to_engine_layout``) or ``"torch"`` (any other dims order: permute and contiguous); from time-major
        model levels ``"ingest"`` (the fused remap of ``vertical.records_to_pressure_device``) or
        ``"relayout+interp"`` (the chain of re-layout and interpolation)."""
        return self._input_path

    @classmethod
    def from_model_levels(cls, ua, va, ta, wap, lat_native, *, plev, ps=None, hyam=None, hybm=None, p0_hybrid=1e5,
                          p_model=None, interp="log", edge="nan", q=None, **kw):
        """TEM diagnostics of fields on model levels (not in the reference, which takes pressure levels only).

        ``ua va ta wap`` (and the tracers ``q``) are ``[ncol][lev][time]`` on the model's levels, top first; ``plev``
        [hPa] are the pressure levels to work on.  The source pressure is hybrid (``ps=`` [ncol][time] in Pa with
        ``hyam=``, ``hybm=`` and ``p0_hybrid=``: p = hyam p0_hybrid + hybm ps) or given point by point
        (``p_model=``); ``interp`` and ``edge`` are ``interp_to_pressure``'s ``method`` and ``edge``.  All fields are
        interpolated on the GPU in one engine call, the model-level device copies are released, and the constructor
        runs on the result with ``plev=`` and everything in ``kw`` (``missing=``, ``min_coverage=``, ``L=`` ...):
        the object equals ``TEMDiagnostics(*interp_to_pressure([ua, va, ta, wap], plev, ...), lat_native, plev=...)``.
        Targets below the surface come out NaN: pass ``missing="mask"`` for those (the default raises, as the
        reference does for NaN input), and ``tracer_mask="own"`` with it when there are tracers: each tracer is then
        fitted under a mask of its own (valid where it, ``va`` and ``wap`` are finite; ``tracer_coverage``).
        ``climatology=True`` next to ``missing="mask"`` needs ``min_time_coverage=v`` (``0 < v <= 1``): the time-mean
        TEM over a mask that varies in time, a point kept where at least that fraction of the record is valid
        (``climatology.py``).  ``time_groups=`` / ``time_weights=`` (grouped and weighted means, next to
        ``climatology=True``) pass through as well and are checked against the record before any device work; next to
        ``missing="mask"`` they need ``min_group_coverage=v`` (``0 < v <= 1``), the masked grouped means.

        Two orders of the axes are served, named by ``dims=`` for raw arrays and by ``.dims`` for labelled ones:
        ``(horz, vert, time)`` as above, and C-contiguous ``(time, vert, horz)`` with ``ps`` as ``(time, horz)`` --
        native model output as it lies in a history file.  The time-major record is never transposed on the host or
        permuted by torch: ``vertical.records_to_pressure_device`` takes it to pressure levels in the engine's layout
        (``input_path`` is ``"ingest"`` or ``"relayout+interp"``, by ``vertical.FUSED_RECORDS``; ``p_model=`` is served
        by the chain), and with ``time_block=n`` one block at a time, host arrays and memmaps through the pinned upload
        ring, so that nothing of whole-record size exists on the device unless the caller put it there.  Any other
        order raises ``ValueError`` before any device work.
        """
        import torch
        from . import vertical
        if kw.get("missing", "raise") not in ("raise", "mask"):
            raise ValueError("missing must be 'raise' or 'mask', got %r" % (kw["missing"],))
        cls._check_tracer_mask(kw.get("tracer_mask"), kw.get("missing", "raise"), q)
        cls._check_lat_bins(kw.get("lat_bins"), kw.get("missing", "raise"))
        wv.check_form(kw.get("wave_form", "generic"), kw.get("wavenumbers") is not None)
        if kw.get("wavenumbers") is not None:
            wv.check_arguments(kw["wavenumbers"], kw.get("lon"), len(lat_native), kw.get("L", 50), missing=kw.get("missing", "raise"),
                               lat_bins=kw.get("lat_bins"), time_block=kw.get("time_block"),
                               climatology=kw.get("climatology", False), wave_form=kw.get("wave_form", "generic"))
        if kw.get("time_bands") is not None:
            tb.check_record(tb.check_arguments(kw["time_bands"], missing=kw.get("missing", "raise"), time_block=kw.get("time_block"),
                                               climatology=kw.get("climatology", False), wavenumbers=kw.get("wavenumbers")),
                            cls._record_times(ua, kw.get("dims"), kw.get("dim_names", DEFAULT_DIMS), kw.get("time"))[0])
        mgc = clim.check_group_coverage(kw.get("min_group_coverage"), kw.get("climatology", False), kw.get("missing", "raise"),
                                        kw.get("time_groups"), kw.get("time_weights"), kw.get("min_time_coverage"))
        clim.check_flag(kw.get("climatology", False), kw.get("missing", "raise"), kw.get("min_time_coverage"), mgc)
        if clim.check_group_flags(kw.get("time_groups"), kw.get("time_weights"), kw.get("climatology", False),
                                  kw.get("missing", "raise"), mgc) is not None:
            clim.resolve_groups(kw.get("time_groups"), kw.get("time_weights"),
                                *cls._record_times(ua, kw.get("dims"), kw.get("dim_names", DEFAULT_DIMS), kw.get("time")))
        qs = [] if q is None else (list(q) if isinstance(q, (list, tuple)) else [q])
        given = [ua, va, ta, wap] + qs
        if cls._model_level_order(given, kw.pop("dims", None), kw.get("dim_names", DEFAULT_DIMS)) == "time-major":
            return cls._from_time_major_levels(given, lat_native, plev, ps, hyam, hybm, p0_hybrid, p_model, interp,
                                               edge, kw)
        outs, plev_asc = vertical._interp(given, plev, ps=ps, hyam=hyam, hybm=hybm, p0=p0_hybrid, p=p_model,
                                          method=interp, edge=edge, device=kw.get("device"), on_device=True)
        # (the model-level device copies died with that call: only the pressure-level tensors are held from here on)
        raw = not containers.is_labeled(ua)
        if raw:
            kw["plev"] = plev_asc
        obj = cls(*outs[:4], lat_native, q=outs[4:] if qs else None, **kw)
        # results come back as the kind that went in, as if the interpolated arrays had been handed over on the host
        v0 = ua if raw else ua.values
        obj._torch_out = isinstance(v0, torch.Tensor)
        if not raw:
            obj._kind = "xarray" if containers.is_xarray(ua) else "labeled"
        return obj

    @staticmethod
    def _record_times(first, dims, dim_names, time):
        """(number of times, time coordinate) of a field as the constructor will see them, from its shape and labels
        alone (host logic only): what ``time_groups`` / ``time_weights`` are checked against before any device work."""
        tname = dim_names.get("time", DEFAULT_DIMS["time"])
        if containers.is_labeled(first):
            d, shape = tuple(first.dims), tuple(first.values.shape)
            if tname in d:
                try:
                    time = np.asarray(containers.coord_of(first, tname))
                except Exception:
                    time = None
        else:
            shape = tuple(first.shape)
            full = (dim_names["horz"], dim_names["vert"], tname)
            d = tuple(dims) if dims is not None else full[:len(shape)]
        nt = int(shape[d.index(tname)]) if tname in d and len(d) == len(shape) else 1
        return nt, (np.asarray(time) if time is not None else np.arange(nt))

    @staticmethod
    def _model_level_order(given, dims, dim_names):
        """``"engine"`` for ``(horz, vert, time)`` / ``(horz, vert)`` input, ``"time-major"`` for ``(time, vert, horz)``;
        ``ValueError`` for mixed kinds and for every other order (host logic only)."""
        labeled = [containers.is_labeled(x) for x in given]
        if any(labeled) and not all(labeled):
            raise ValueError("fields must all be of the same kind")
        horz, time = dim_names["horz"], dim_names.get("time", DEFAULT_DIMS["time"])
        orders = set()
        for x in given:
            d = tuple(x.dims) if labeled[0] else (None if dims is None else tuple(dims))
            if d is None or (len(d) in (2, 3) and d[0] == horz and (len(d) == 2 or d[2] == time) and horz not in d[1:]):
                orders.add("engine")
            elif len(d) == 3 and d[0] == time and d[2] == horz and d[1] not in (time, horz):
                orders.add("time-major")
            else:
                raise ValueError("from_model_levels takes its fields as (%s, vert, %s) or as C-contiguous (%s, vert, %s) "
                                 "with ps as (%s, %s); dims %r are neither, and no array is permuted behind the "
                                 "caller's back" % (horz, time, time, horz, time, horz, d))
        if len(orders) != 1:
            raise ValueError("the fields of from_model_levels must all have the same order of dims")
        return orders.pop()

    @classmethod
    def _from_time_major_levels(cls, given, lat_native, plev, ps, hyam, hybm, p0_hybrid, p_model, interp, edge, kw):
        """``from_model_levels`` for C-contiguous ``(time, vert, horz)`` fields: everything that can be refused is
        refused on the host, then the constructor runs over a block source of ``vertical``."""
        import torch
        from . import _vert, vertical
        accepted = ("the accepted orders are (horz, vert, time) and C-contiguous (time, vert, horz) with ps as "
                    "(time, horz)")
        if interp not in _vert.METHODS:
            raise ValueError("method must be 'log' or 'linear', got %r" % (interp,))
        if edge not in _vert.EDGES:
            raise ValueError("edge must be 'nan' or 'hold', got %r" % (edge,))
        if (ps is None) == (p_model is None):
            raise ValueError("give exactly one of ps= (hybrid levels, with hyam= and hybm=) and p_model= (pressure of "
                             "every point)")
        hybrid = ps is not None
        if hybrid and (hyam is None or hybm is None):
            raise ValueError("hybrid levels (ps=) need hyam= and hybm=")
        plev_asc = vertical._check_plev(plev)
        time_block = layout.check_time_block(kw.get("time_block"))
        first = given[0]
        labeled = containers.is_labeled(first)
        vals = [x.values if labeled else x for x in given]
        pin = ps if hybrid else p_model
        pin = pin.values if containers.is_labeled(pin) else pin
        fdt = {"float32": torch.float32, "float64": torch.float64}

        def tdtype(v):
            return fdt.get(str(v.dtype).replace("torch.", ""))
        for i, v in enumerate(vals + [pin]):
            what = "field %d" % i if i < len(vals) else ("ps" if hybrid else "p_model")
            if not isinstance(v, (np.ndarray, torch.Tensor)):
                raise ValueError("%s must be a numpy array, a torch tensor or a labelled array of one" % what)
            if tdtype(v) is None:
                raise ValueError("%s of time-major input must be float64 or float32, got %s" % (what, v.dtype))
            contiguous = v.flags.c_contiguous if isinstance(v, np.ndarray) else v.is_contiguous()
            if not contiguous:
                raise ValueError("%s is not C-contiguous: time-major input is taken as it lies (%s)" % (what, accepted))
        shape = tuple(vals[0].shape)
        if len(shape) != 3:
            raise ValueError("time-major fields must be (time, vert, horz), got %d dims" % len(shape))
        nt, nlev, ncol = (int(n) for n in shape)
        for i, v in enumerate(vals):
            if tuple(v.shape) != shape:
                raise ValueError("field %d has shape %s, expected %s" % (i, tuple(v.shape), shape))
        if nlev < 2 or ncol < 1 or nt < 1:
            raise ValueError("fields need at least one time, two levels and one column, got shape %s" % (shape,))
        want = (nt, ncol) if hybrid else shape
        if tuple(pin.shape) != want:
            raise ValueError("%s has shape %s, expected %s for time-major fields (%s)"
                             % ("ps" if hybrid else "p_model", tuple(pin.shape), want, accepted))
        if hybrid:
            hyam = np.asarray(hyam, dtype=np.float64).ravel()
            hybm = np.asarray(hybm, dtype=np.float64).ravel()
            if hyam.shape[0] != nlev or hybm.shape[0] != nlev:
                raise ValueError("hyam / hybm have %d / %d entries but the fields have %d levels"
                                 % (hyam.shape[0], hybm.shape[0], nlev))
            if not (np.all(np.isfinite(hyam)) and np.all(np.isfinite(hybm)) and np.isfinite(p0_hybrid)):
                raise ValueError("hyam, hybm and p0 must be finite")
        on_device = [isinstance(v, torch.Tensor) and v.is_cuda for v in vals + [pin]]
        if hybrid and not any(on_device):     # host record: min / max of the finite ps, read block-wise
            rng = vertical.finite_range(pin)
            if rng is not None:
                vertical.check_hybrid_monotone(hyam, hybm, float(p0_hybrid), *rng)

        # ---- device work from here on ----
        device = kw.get("device")
        dev = device if isinstance(device, torch.device) else torch.device("cuda", int(device or 0))
        tdt = [tdtype(v) for v in vals]
        work = torch.float32 if set(tdt) == {torch.float32} else torch.float64
        arrays = vals + [pin]
        host_fed = not any(on_device)
        if not host_fed:
            arrays = [(a if isinstance(a, torch.Tensor) else torch.as_tensor(a)).to(dev) for a in arrays]
            if hybrid:
                rng = vertical.finite_range(arrays[-1])
                if rng is not None:
                    vertical.check_hybrid_monotone(hyam, hybm, float(p0_hybrid), *rng)
        # a blocked host-fed run takes the fused call whatever the gate says: the chain's intermediate would be one
        # more model-level block on the device, which is what the blocks are there to avoid
        path = "fused" if host_fed and time_block is not None and hybrid else None
        step = vertical._RecordStep(len(vals), plev_asc * 100.0, hyam, hybm, p0_hybrid, interp, edge, work, not hybrid, path)
        source = vertical.HostRecordBlocks(arrays, dev, step) if host_fed else vertical.DeviceRecordBlocks(arrays, step)
        # the constructor sees the shapes and dtypes of the pressure-level fields; the source brings their values
        stand_in = [torch.empty((ncol, plev_asc.size, nt), dtype=dt, device="meta") for dt in tdt]
        kw["plev"] = plev_asc
        if labeled:
            tname = first.dims[0]
            try:
                kw.setdefault("time", np.asarray(containers.coord_of(first, tname)))
            except Exception:
                pass
        _pending.source = source
        try:
            obj = cls(*stand_in[:4], lat_native, q=stand_in[4:] if len(stand_in) > 4 else None, **kw)
        finally:
            _pending.source = None
        obj._torch_out = isinstance(vals[0], torch.Tensor)
        if labeled:
            obj._kind = "xarray" if containers.is_xarray(first) else "labeled"
        return obj

    @staticmethod
    def _check_tracer_mask(tracer_mask, missing, q):
        """``tracer_mask`` as given (ValueError for an unknown value, or for "own" without ``missing="mask"``);
        tracers next to ``missing="mask"`` without it keep raising NotImplementedError.  Host logic only."""
        if tracer_mask not in (None, "own"):
            raise ValueError("tracer_mask must be None or 'own', got %r" % (tracer_mask,))
        if tracer_mask == "own" and missing != "mask":
            raise ValueError("tracer_mask='own' needs missing='mask': in the default mode a tracer has no mask")
        if missing == "mask" and q is not None and tracer_mask is None:
            raise NotImplementedError("missing='mask' does not support tracers (q=) unless tracer_mask='own' is given: "
                                      "a masked tracer has a mask of its own (valid where q, va and wap are all "
                                      "finite) and a coverage of its own (tracer_coverage); or fill or drop the "
                                      "tracer's missing values, or run it separately with missing='raise'")
        return tracer_mask

    # ------------------------------------------------------------------------------------------
    def _config_dims(self):
        """Validation and reshaping of tem_diagnostics.py:266-405 (host side only)."""
        import torch
        self.ncolname = self.dim_names["horz"]
        self.plevname = self.dim_names["vert"]
        try:
            self.timename = self.dim_names["time"]
        except KeyError:
            self.timename = DEFAULT_DIMS["time"]
        self.data_dims = (self.ncolname, self.plevname, self.timename)

        # tracers (tem_diagnostics.py:281-301): a labelled array / raw array, or a list of them
        if self.q is not None:
            if not isinstance(self.q, list):
                self.q = [self.q]
            ok = all(containers.is_labeled(x) or isinstance(x, (np.ndarray, torch.Tensor)) for x in self.q)
            if not ok or len(self.q) == 0:
                raise RuntimeError("tracers q must be passed as an xarray DataArray, or"
                                   "a list of xarray DataArrays")
            self.ntrac = len(self.q)
        else:
            self.q = []
            self.ntrac = 0
        self._q_out_file = [None] * self.ntrac
        for i, x in enumerate(self.q):
            self._in["q{}".format(i)] = x

        lat = self.lat_native
        self._lat_native_np = np.asarray(lat.values if containers.is_labeled(lat) else
                                         (lat.detach().cpu().numpy() if hasattr(lat, "detach") else lat),
                                         dtype=np.float64)
        nlat = self._lat_native_np.shape[0]

        labeled = [containers.is_labeled(v) for v in self._in.values()]
        if any(labeled) and not all(labeled):
            raise RuntimeError("Input data for args ua, va, ta, wap (and q) must all be of the same kind")
        self._kind = "raw"
        if all(labeled):
            self._kind = "xarray" if containers.is_xarray(self._in["ua"]) else "labeled"

        vals, raw, tmajor = {}, {}, {}
        for var, dat in self._in.items():
            if self._kind == "raw":
                if not (isinstance(dat, np.ndarray) or isinstance(dat, torch.Tensor)):
                    raise RuntimeError("Input data for arg '{}' must be an xarray DataArray".format(var))   # :313
                ddims = tuple(self._raw_dims) if self._raw_dims is not None else self.data_dims[:dat.ndim]
                v = dat
            else:
                ddims = tuple(dat.dims)
                v = dat.values
            if self.ncolname not in ddims:                                                    # :316-318
                raise RuntimeError("Input data {} does not contain dim {}".format(var, self.ncolname))
            if v.shape[ddims.index(self.ncolname)] != nlat:                                   # :320-323
                raise RuntimeError("Dimension {} in variable {} is length {}, but input parameter lat is "
                                   "length {}; these must match!".format(
                                       self.ncolname, var, v.shape[ddims.index(self.ncolname)], nlat))
            if len(ddims) < 2 or len(ddims) > 3:                                              # :326-329
                raise RuntimeError("Input data has {0} dims, expected either 2 ({1}, {2}) or 3 ({1}, {2}, {3})"
                                   .format(len(ddims), self.ncolname, self.plevname, self.timename))
            raw[var] = v
            tmajor[var] = layout.is_time_major(ddims, self.data_dims, v)
            t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
            if self.timename not in ddims:                  # 2-D input: add a length-1 time axis (:332-335)
                t = t.unsqueeze(-1)
                ddims = ddims + (self.timename,)
            if self.plevname not in ddims:
                raise RuntimeError("Input data {} does not contain dim {}".format(var, self.plevname))
            perm = [ddims.index(n) for n in self.data_dims]                                   # :343-353
            vals[var] = t.permute(*perm)

        ua = self._in["ua"]
        # ---- coordinates (tem_diagnostics.py:360-367) ----
        if self._kind == "raw":
            if self._raw_plev is None:
                raise RuntimeError("raw array inputs need plev= (pressure levels in hPa)")
            plev = np.asarray(self._raw_plev, dtype=np.float64)
            nt = vals["ua"].shape[2]
            time = np.asarray(self._raw_time) if self._raw_time is not None else np.arange(nt)
        else:
            plev = np.asarray(containers.coord_of(ua, self.plevname), dtype=np.float64)
            time = containers.coord_of(ua, self.timename) if self.timename in ua.dims else np.zeros(1)
        self.NCOL, self.NLEV, self.NT = (int(s) for s in vals["ua"].shape)
        if plev.shape[0] != self.NLEV:
            raise RuntimeError("plev has {} entries but the data have {} levels".format(plev.shape[0], self.NLEV))
        for var in [v for v in vals if v != "ua"]:
            if tuple(vals[var].shape) != tuple(vals["ua"].shape):
                raise RuntimeError("Input data {} has shape {}, expected {}".format(
                    var, tuple(vals[var].shape), tuple(vals["ua"].shape)))

        # ---- pressure direction: model top first (tem_diagnostics.py:369-382) ----
        # (time-major input: the GPU re-layout reverses the levels on its way, no flipped copy is made)
        relayout = all(tmajor.values()) and all(v.dtype in (torch.float32, torch.float64) for v in vals.values())
        if relayout and self.time_block is None:
            work_name = "float32" if all(v.dtype == torch.float32 for v in vals.values()) else "float64"
            relayout = layout.WHOLE_RUN_KERNEL[work_name]
        self._input_path = "relayout" if relayout else "torch"
        flip = bool(plev[0] > plev[-1])
        if flip:
            if not relayout:
                vals = {k: torch.flip(v, dims=(1,)) for k, v in vals.items()}
            plev = plev[::-1].copy()
        self.plev = plev
        self.time = time
        self.p = self.plev * 100                                                              # :385
        self._p_np = np.asarray(self.p, dtype=np.float64)

        # ---- zonal-mean latitudes (tem_diagnostics.py:387-398) ----
        tol = 1e-6
        assert (180 / self.zm_dlat).is_integer(), "180 must be divisible by dlat_out"
        self._lat_zm = np.arange(-90, 90 + self.zm_dlat, self.zm_dlat)
        if self._lat_zm[-1] > 90 + tol:
            self._lat_zm = self._lat_zm[:-1]
        if not self.zm_pole_points:
            self._lat_zm = (self._lat_zm[1:] + self._lat_zm[:-1]) / 2
        self.ZM_N = len(self._lat_zm)
        self._f_zm = 2 * Om * np.sin(self._lat_zm * np.pi / 180)                              # :401
        self._coslat_zm = np.cos(self._lat_zm * np.pi / 180)                                  # :402
        self.lat, self.coslat = self._lat_zm, self._coslat_zm
        self.f = self._f_zm[:, np.newaxis, np.newaxis]

        # ---- grouped and weighted time means (climatology.py): labels and weights against the record, on the host ----
        if self._group_args is not None:
            self._groups = clim.resolve_groups(*self._group_args, self.NT, self.time)

        # ---- EP flux by time scale (timebands.py): the record against the filter's length, on the host ----
        if self._band_args is not None:
            tb.check_record(self._band_args, self.NT)

        # ---- device residency: contiguous [ncol][plev][time], one dtype ----
        dts = {v.dtype for v in vals.values()}
        self._in_dtype = {k: v.dtype for k, v in vals.items()}
        work = torch.float32 if dts == {torch.float32} else torch.float64
        dev = torch.device("cuda", int(self._device) if not isinstance(self._device, torch.device)
                           else (self._device.index or 0))
        self._torch_out = isinstance(self._in["ua"], torch.Tensor) or (
            self._kind != "raw" and isinstance(self._in["ua"].values, torch.Tensor))
        self._work_dtype = work
        names = ["ua", "va", "ta", "wap"] + ["q{}".format(i) for i in range(self.ntrac)]
        self._block_source = None
        if self._given_source is not None:
            # time-major model levels (from_model_levels): the inputs are shapes only, the source brings the fields
            self._dev_fields, self._dev_q = None, None
            self._block_source, self._given_source = self._given_source, None
            self._input_path = self._block_source.input_path
        elif self.time_block is not None:
            # blocked run: nothing is made resident here, _run_blocked brings one block at a time
            self._dev_fields, self._dev_q = None, None
            srcs = [raw[k] for k in names]
            if not relayout:
                self._block_source = layout.TorchBlocks([vals[k] for k in names], dev, work)
            elif all(isinstance(x, np.ndarray) or not x.is_cuda for x in srcs):
                self._block_source = layout.HostBlocks(srcs, dev, flip, work)
            else:
                srcs = [(x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(dev) for x in srcs]
                self._block_source = layout.DeviceBlocks(srcs, flip, work)
        elif relayout:
            # time-major input goes up as it lies; the re-layout makes the engine's copy, flip and widening included.
            # Fields already on the device move in one launch; a host field goes up, is re-laid out and released
            # before the next one, so the peak is the record plus one field, not twice the record.
            up = [raw[k] if isinstance(raw[k], torch.Tensor) else torch.as_tensor(np.asarray(raw[k])) for k in names]
            if all(x.is_cuda and x.device == dev for x in up):
                outs = layout.to_engine_layout(up, flip_lev=flip, dtype=work)
            else:
                with torch.cuda.device(dev):
                    outs = list(torch.empty((len(up), self.NCOL, self.NLEV, self.NT), dtype=work, device=dev).unbind(0))
                for x, o in zip(up, outs):
                    layout.to_engine_layout([x.to(dev)], flip_lev=flip, dtype=work, out=[o])
            del up
            self._dev_fields, self._dev_q = outs[:4], outs[4:]
        else:
            self._dev_fields = [vals[k].to(device=dev, dtype=work).contiguous() for k in ("ua", "va", "ta", "wap")]
            self._dev_q = [vals["q{}".format(i)].to(device=dev, dtype=work).contiguous() for i in range(self.ntrac)]
        self._tracer_names = [getattr(x, "name", None) for x in self.q]

    # ------------------------------------------------------------------------------------------
    def _np_dtype(self, var):
        import torch
        if isinstance(var, tuple):           # numpy promotion of a product of two inputs
            return np.result_type(*[self._np_dtype(v) for v in var]).type
        return {torch.float32: np.float32, torch.float64: np.float64}.get(self._in_dtype[var], np.float64)

    def _wrap(self, t, name, src_var, native=False, force64=False, time=None):
        """Label a device result; cast like the reference's astype.  ``time``: the time coordinate when
        it is not the input's (the time-mean results of ``climatology``)."""
        import torch
        dt = np.float64 if (force64 or name in _F64_ALWAYS) else self._np_dtype(src_var)
        dt = np.float64 if dt == np.float64 else np.float32
        tdt = torch.float64 if dt == np.float64 else torch.float32
        t = t.to(tdt)
        vals = t if self._torch_out else t.cpu().numpy()
        if self._kind == "raw":
            return vals
        first = self.ncolname if native else "lat"
        dims = (first, self.plevname, self.timename)
        coords = {self.plevname: self.plev, self.timename: self.time if time is None else time}
        if not native:
            coords["lat"] = self._lat_zm
        return containers.make_like(self._kind, vals, dims, coords, name)

    def _zonal(self, name, src_var):
        return self._wrap(self._zon[_lib.ZONAL_NAMES.index(name)], name, src_var)

    def _result(self, name, src_var):
        return self._wrap(self._res[_lib.RESULT_NAMES.index(name)], name, src_var)

    def _native(self, name, src_var):
        self._refuse_native(name)
        if self._eddy is None:                        # lazily materialised [ncol][plev][time] fields
            self._eddy = self.ZM._plan.tem_eddy(*self._dev_fields)
        return self._wrap(self._eddy[name], name, src_var, native=True)

    def iter_native(self, names=_lib.EDDY_NAMES, chunk_cols=65536):
        """Stream the native-grid attributes (``up vp thetap wapp upvp upwapp vptp``,
        tem_diagnostics.py:420-433) in blocks of columns instead of materialising ``[ncol][plev][time]``
        arrays whole: yields ``(col0, col1, {name: ndarray[col1 - col0, plev, time]})`` with the dtype the
        corresponding property would have.  Device memory: one block of seven arrays."""
        self._refuse_native("iter_native")
        return self._iter_native(names, chunk_cols)

    def _iter_native(self, names, chunk_cols):
        chunk = max(16, (int(chunk_cols) // 16) * 16)
        src = {"up": "ua", "vp": "va", "thetap": "ta", "wapp": "wap", "upvp": "ua", "upwapp": "ua", "vptp": "va"}
        for c0 in range(0, self.NCOL, chunk):
            c1 = min(self.NCOL, c0 + chunk)
            blk = self.ZM._plan.tem_eddy_rows(*self._dev_fields, c0, c1 - c0, names=tuple(names))
            out = {}
            for n, v in blk.items():
                a = v.cpu().numpy()
                dt = np.float64 if n in _F64_ALWAYS else self._np_dtype(src[n])
                out[n] = a.astype(np.float64 if dt == np.float64 else np.float32, copy=False)
            yield c0, c1, out

    # ---- getters (tem_diagnostics.py:412-487) ----
    ub = property(lambda s: s._zonal("ub", "ua"))

    @property
    def coverage(self):
        """missing="mask": the spectral zonal-mean valid fraction of the run on the zonal grid (labelled like
        ``ub``, float64); outputs are NaN where it is below ``min_coverage``.  None in the default mode."""
        if self._cov is None:
            return None
        return self._wrap(self._cov, "coverage", "ua", force64=True)
    vb = property(lambda s: s._zonal("vb", "va"))
    thetab = property(lambda s: s._zonal("thetab", "ta"))
    wapb = property(lambda s: s._zonal("wapb", "wap"))
    up = property(lambda s: s._native("up", "ua"))
    vp = property(lambda s: s._native("vp", "va"))
    thetap = property(lambda s: s._native("thetap", "ta"))
    wapp = property(lambda s: s._native("wapp", "wap"))
    upvp = property(lambda s: s._native("upvp", "ua"))
    upwapp = property(lambda s: s._native("upwapp", "ua"))
    vptp = property(lambda s: s._native("vptp", "va"))
    upvpb = property(lambda s: s._zonal("upvpb", "ua"))
    upwappb = property(lambda s: s._zonal("upwappb", "ua"))
    vptpb = property(lambda s: s._zonal("vptpb", "va"))
    dub_dp = property(lambda s: s._zonal("dub_dp", "ua"))
    dthetab_dp = property(lambda s: s._zonal("dthetab_dp", "ta"))
    ubcoslat = property(lambda s: s._zonal("ubcoslat", "ua"))
    dubcoslat_dlat = property(lambda s: s._zonal("dubcoslat_dlat", "ua"))
    psicoslat = property(lambda s: s._zonal("psicoslat", "ta"))
    dpsicoslat_dlat = property(lambda s: s._zonal("dpsicoslat_dlat", "ta"))
    int_vbdp = property(lambda s: s._zonal("int_vbdp", "va"))
    psi = property(lambda s: s._zonal("psi", "ta"))
    dpsi_dp = property(lambda s: s._zonal("dpsi_dp", "ta"))
    # ---- tracer getters: lists, one entry per tracer (tem_diagnostics.py:458-475) ----
    def _tzonal(self, name, src, force64=False):
        k = _lib.TRACER_ZONAL_NAMES.index(name)
        return [self._wrap(self._tzon[i][k], name, src(i), force64=force64) for i in range(self.ntrac)]

    def _tnative(self, name, src):
        self._refuse_native(name)
        out = []
        for i in range(self.ntrac):
            if self._teddy[i] is None:
                plan = self.ZM._plan
                run, eddy = plan.tracer_run, plan.tracer_eddy
                if self.missing == "mask":      # tracer_mask="own"
                    run, eddy = plan.tracer_run_masked, plan.tracer_eddy_masked
                if self._last_tracer != i:      # the plan holds the coefficients of one tracer at a time
                    run(self._dev_q[i], self._dev_fields[1], self._dev_fields[3])
                    self._last_tracer = i
                self._teddy[i] = eddy(self._dev_q[i], self._dev_fields[1], self._dev_fields[3])
            out.append(self._wrap(self._teddy[i][name], name, src(i), native=True))
        return out

    qb = property(lambda s: s._tzonal("qb", lambda i: "q%d" % i))
    qpvpb = property(lambda s: s._tzonal("qpvpb", lambda i: ("q%d" % i, "va")))
    qpwappb = property(lambda s: s._tzonal("qpwappb", lambda i: ("q%d" % i, "wap")))
    dqb_dp = property(lambda s: s._tzonal("dqb_dp", lambda i: "q%d" % i))
    qbcoslat = property(lambda s: s._tzonal("qbcoslat", lambda i: "q%d" % i, force64=True))
    dqbcoslat_dlat = property(lambda s: s._tzonal("dqbcoslat_dlat", lambda i: "q%d" % i, force64=True))
    qp = property(lambda s: s._tnative("qp", lambda i: "q%d" % i))
    qpvp = property(lambda s: s._tnative("qpvp", lambda i: ("q%d" % i, "va")))
    qpwapp = property(lambda s: s._tnative("qpwapp", lambda i: ("q%d" % i, "wap")))

    @property
    def theta(self):
        """theta = T (p0/p)^k (tem_diagnostics.py:498); recovered as thetap + its native zonal mean
        would cost a sweep, so it is formed from the same per-level scale the engine fuses."""
        import torch
        self._refuse_native("theta")
        if self._theta is None:
            from .constants import k
            scale = torch.as_tensor((float(self.p0) / self._p_np) ** k, device=self._dev_fields[2].device)
            self._theta = self._dev_fields[2].to(torch.float64) * scale[None, :, None]
        return self._wrap(self._theta, "THETA", "ta", native=True, force64=True)

    @property
    def out_file(self):
        if self._out_file is None:
            warnings.warn("'out_file' is not set until to_netcdf() is called")
        return self._out_file

    @property
    def q_out_file(self):
        if len(self._q_out_file) == 0:
            warnings.warn("'q_out_file' is emtpy; no tracers currently present")
        if self._q_out_file.count(None) == self.ntrac:
            warnings.warn("'q_out_file' is not set until q_to_netcdf() is called")
        return self._q_out_file

    # ---- the ten diagnostics (tem_diagnostics.py:615-797), each cast to its input's dtype ----
    def vtem(self): return self._result("vtem", "va")                  # noqa: E704
    def omegatem(self): return self._result("omegatem", "wap")         # noqa: E704
    def wtem(self): return self._result("wtem", "wap")                 # noqa: E704
    def psitem(self): return self._result("psitem", "va")              # noqa: E704
    def epfy(self): return self._result("epfy", "ua")                  # noqa: E704
    def epfz(self): return self._result("epfz", "ua")                  # noqa: E704
    def epdiv(self): return self._result("epdiv", "ua")                # noqa: E704
    def utendepfd(self): return self._result("utendepfd", "ua")        # noqa: E704
    def utendvtem(self): return self._result("utendvtem", "ua")        # noqa: E704
    def utendwtem(self): return self._result("utendwtem", "ua")        # noqa: E704

    # ---- tracer TEM (Abalos+ 2017), tem_diagnostics.py:801-991 ----
    def _tracer_result(self, name, qi):
        if qi is None and self.ntrac == 1:
            qi = 0
        elif qi is None and self.ntrac > 1:                                   # :815-816 ...
            raise RuntimeError("qi must be passed to {}() when len(q) > 1!".format(name))
        if self.ntrac == 0:
            raise RuntimeError("no tracers present (argument `q` not passed at object construction)")
        return self._wrap(self._tres[qi][_lib.TRACER_RESULT_NAMES.index(name)], name, "q%d" % qi)

    def tracer_coverage(self, qi=None):
        """``tracer_mask="own"``: the spectral zonal-mean valid fraction of tracer ``qi`` on the zonal grid -- valid
        where ``q``, ``va`` and ``wap`` are all finite -- labelled like ``coverage`` (float64); the tracer's outputs
        are NaN where it is below ``min_coverage``.  None in the default mode."""
        if qi is None and self.ntrac > 1:
            raise RuntimeError("qi must be passed to tracer_coverage() when len(q) > 1!")
        if self.ntrac == 0:
            raise RuntimeError("no tracers present (argument `q` not passed at object construction)")
        if not self._tcov:
            return None
        return self._wrap(self._tcov[qi or 0], "tracer_coverage", "q%d" % (qi or 0), force64=True)

    def etfy(self, qi=None): return self._tracer_result("etfy", qi)               # noqa: E704
    def etfz(self, qi=None): return self._tracer_result("etfz", qi)               # noqa: E704
    def etdiv(self, qi=None): return self._tracer_result("etdiv", qi)             # noqa: E704
    def qtendetfd(self, qi=None): return self._tracer_result("qtendetfd", qi)     # noqa: E704
    def qtendvtem(self, qi=None): return self._tracer_result("qtendvtem", qi)     # noqa: E704
    def qtendwtem(self, qi=None): return self._tracer_result("qtendwtem", qi)     # noqa: E704

    def results(self):
        return {n: getattr(self, n)() for n in _lib.RESULT_NAMES}

    # ---- I/O (tem_diagnostics.py:995-1041): needs xarray + a NetCDF back end ----
    def to_netcdf(self, loc=os.getcwd(), prefix=None, include_attrs=False):
        prefix = "{}_".format(prefix) if prefix is not None else ""
        filename = "{}TEM_{}_{}_L{}.nc".format(prefix, self.ZM.grid_name, self.ZM.grid_out_name, self.L)
        self._out_file = "{}/{}".format(loc, filename)
        names = {}
        if include_attrs:
            self._refuse_native("to_netcdf(include_attrs=True)")
        if include_attrs:   # (sic) key 'wawpp' as in tem_diagnostics.py:1011
            names = {"ub": "ub", "up": "up", "vb": "vb", "vp": "vp", "thetab": "thetab", "thetap": "thetap",
                     "wapb": "wapb", "wawpp": "wapp", "upvp": "upvp", "upvpb": "upvpb", "upwapp": "upwapp",
                     "upwappb": "upwappb", "vptp": "vptp", "vptpb": "vptpb", "dub_dp": "dub_dp",
                     "dthetab_dp": "dthetab_dp", "ubcoslat": "ubcoslat", "dubcoslat_dlat": "dubcoslat_dlat",
                     "psi": "psi", "psicoslat": "psicoslat", "dpsicoslat_dlat": "dpsicoslat_dlat",
                     "dpsi_dp": "dpsi_dp", "int_vbdp": "int_vbdp"}
        items = dict({k: getattr(self, v) for k, v in names.items()},
                     **{n: getattr(self, n)() for n in _lib.RESULT_NAMES})
        self._write_nc(self._out_file, items)
        return self._out_file

    def _write_nc(self, path, items):
        """xarray when importable (like the reference); otherwise NetCDF-3 through scipy (ncio.py)."""
        try:
            import xarray as xr
        except ImportError:
            xr = None
        if xr is not None:   # pragma: no cover - xarray is absent from this image
            xr.Dataset({k: self._as_xr(v) for k, v in items.items()}).to_netcdf(path)
            return
        from . import ncio
        variables = {}
        for k, v in items.items():
            arr = ncio._np(v)
            native = arr.shape[0] == self.NCOL and arr.shape[0] != len(self.lat)
            dims = v.dims if containers.is_labeled(v) else (("ncol" if native else "lat"), self.plevname, self.timename)
            variables[k] = (tuple(dims), arr, getattr(v, "attrs", None))
        coords = {"lat": np.asarray(self.lat, dtype=np.float64), self.plevname: np.asarray(self.plev, dtype=np.float64)}
        t = np.asarray(self.time)
        if t.dtype.kind in "fiu":
            coords[self.timename] = t.astype(np.float64)
        ncio.write_dataset(path, variables, coords)

    def _as_xr(self, x):
        import xarray as xr
        if isinstance(x, xr.DataArray):
            return x
        v = x.values if containers.is_labeled(x) else x
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        dims = x.dims if containers.is_labeled(x) else ("lat", self.plevname, self.timename)
        return xr.DataArray(v, dims=dims)

    def q_to_netcdf(self, loc=os.getcwd(), qi=None, prefix=None, include_attrs=False):
        """tem_diagnostics.py:1045-1103 (file naming and variable set; needs xarray + NetCDF)."""
        assert self.ntrac > 0, "No tracers to output (argument `q` not passed at object construction)"
        prefix = "{}_".format(prefix) if prefix is not None else ""
        names = [n if n is not None else "q{}".format(i) for i, n in enumerate(self._tracer_names)]
        idx = range(self.ntrac) if qi is None else [qi]
        for i in idx:
            items = {n: getattr(self, n)(i) for n in _lib.TRACER_RESULT_NAMES}
            if include_attrs:   # (sic) key 'dqp_dp' as in tem_diagnostics.py:1081
                items = dict({"qpvp": self.qpvp[i], "qpwapp": self.qpwapp[i], "qpvpb": self.qpvpb[i],
                              "qpwappb": self.qpwappb[i], "dqp_dp": self.dqb_dp[i], "qbcoslat": self.qbcoslat[i],
                              "dqbcoslat_dlat": self.dqbcoslat_dlat[i]}, **items)
            self._q_out_file[i] = "{}/{}TEM_{}_{}_L{}_TRACER-{}.nc".format(
                loc, prefix, self.ZM.grid_name, self.ZM.grid_out_name, self.L, names[i])
            self._write_nc(self._q_out_file[i], items)
        return self._q_out_file
