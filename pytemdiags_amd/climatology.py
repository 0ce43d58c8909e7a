"""Time-mean TEM with stationary and transient eddy fluxes (``TEMDiagnostics(..., climatology=True)``; not in the
reference, which gives one TEM state per snapshot).

With ``[.]`` the uniform mean over the ``NT`` snapshots of the record and an overbar the spectral zonal mean:

  * mean state        ``[ub] [vb] [thetab] [wapb]``: the time means of the per-snapshot zonal means (the operator is
    linear and does not depend on time, so these are the zonal means of the time-mean fields);
  * total fluxes      the time means of the per-snapshot ``upvpb upwappb vptpb``;
  * stationary fluxes ``upvpb upwappb vptpb`` of a TEM run on the time-mean native-grid fields (``nt = 1``): the eddies
    of the time-mean flow;
  * transient fluxes  total - stationary: the time mean of the zonal-mean products of the deviations from the time mean.

Each of the three result sets (``total``, ``stationary``, ``transient``) is the unchanged epilogue of a TEM run applied
to the same mean state and that set's three fluxes: ten results and sixteen zonal intermediates of shape
``(lat, plev, 1)``, the time coordinate the mean of the input's.  ``epfy epfz epdiv utendepfd`` are linear and
homogeneous in the fluxes, so stationary + transient = total for those four; the other six carry the mean-state term in
every set.

Device work: the time sum of the four resident fields (``engine.Plan.time_sum``, fused into the block loop of a blocked
run), one TEM run on the fp64 mean fields, and three epilogues on supplied zonal means
(``engine.Plan.tem_from_zonal_means``); all on the plan of the ordinary run, which runs last and leaves the plan's
state as an object built without ``climatology`` has it.
"""
from __future__ import annotations

import numpy as np

from . import _lib

# Whether the time sum of fields of a work dtype goes through the HIP kernel (temxc_time_sum) or through
# torch.sum(x, -1, dtype=float64).  Set from tools/clim_bench.py (profiles/clim_bench_mi355x.json): the kernel is on
# for a dtype where it is faster than torch at ne120 x 72 x 30.  The engine method is always the kernel.
TIME_SUM_KERNEL = {"float64": True, "float32": True}

FLUX_NAMES = ("upvpb", "upwappb", "vptpb")
LINEAR_RESULTS = ("epfy", "epfz", "epdiv", "utendepfd")
SET_NAMES = ("total", "stationary", "transient")

# the input whose dtype a quantity is cast to (as the getters of TEMDiagnostics have it)
_RESULT_SRC = {"vtem": "va", "omegatem": "wap", "wtem": "wap", "psitem": "va", "epfy": "ua", "epfz": "ua",
               "epdiv": "ua", "utendepfd": "ua", "utendvtem": "ua", "utendwtem": "ua"}
_ZONAL_SRC = {"ub": "ua", "vb": "va", "thetab": "ta", "wapb": "wap", "upvpb": "ua", "upwappb": "ua", "vptpb": "va",
              "dub_dp": "ua", "dthetab_dp": "ta", "ubcoslat": "ua", "dubcoslat_dlat": "ua", "psi": "ta",
              "psicoslat": "ta", "dpsicoslat_dlat": "ta", "dpsi_dp": "ta", "int_vbdp": "va"}
_NAN_MESSAGE = ("Variable has nans! Spectral zonal averager cannot handle nans; "
                "please replace or remove them")


def check_flag(climatology, missing):
    """``climatology`` as a bool; ValueError for anything else and next to ``missing="mask"`` (no device needed)."""
    if not isinstance(climatology, (bool, np.bool_)):
        raise ValueError("climatology must be True or False, got %r" % (climatology,))
    if climatology and missing == "mask":
        raise ValueError("climatology=True and missing='mask' exclude each other: a time mean over a mask that varies "
                         "in time needs a contract of its own")
    return bool(climatology)


def mean_time(time):
    """The mean of a time coordinate as a length-1 array (numbers, datetime64; anything else keeps its first entry)."""
    t = np.asarray(time)
    if t.size == 0:
        return np.zeros(1)
    if t.dtype.kind in "iuf":
        return np.array([t.astype(np.float64).mean()])
    if t.dtype.kind in "Mm":
        d = t - t[0]
        return np.array([t[0] + np.int64(np.rint(d.astype("int64").mean())).astype(d.dtype)])
    return t[:1].copy()


class ResultSet:
    """One of ``total``, ``stationary``, ``transient``: the ten result methods, the sixteen zonal attributes and
    ``results()`` of ``TEMDiagnostics``, each ``(lat, plev, 1)``, wrapped and cast by the owner's own wrapping code."""

    def __init__(self, owner, name, res, zon, time):
        self.name = name
        self._owner, self._res, self._zon, self._time = owner, res, zon, time

    def _result(self, name):
        return self._owner._wrap(self._res[_lib.RESULT_NAMES.index(name)], name, _RESULT_SRC[name], time=self._time)

    def _zonal(self, name):
        return self._owner._wrap(self._zon[_lib.ZONAL_NAMES.index(name)], name, _ZONAL_SRC[name], time=self._time)

    def results(self):
        return {n: self._result(n) for n in _lib.RESULT_NAMES}


for _n in _lib.RESULT_NAMES:
    setattr(ResultSet, _n, (lambda n: lambda self: self._result(n))(_n))
for _n in _lib.ZONAL_NAMES:
    setattr(ResultSet, _n, property((lambda n: lambda self: self._zonal(n))(_n)))
del _n


class TEMClimatology:
    """``tem.climatology``: the three result sets of the time-mean TEM (module docstring).  ``nt`` is the number of
    snapshots averaged, ``time`` the mean of their time coordinate, ``time_sum_path`` ``"kernel"`` or ``"torch"``."""

    def __init__(self, owner, sets, nt, time, time_sum_path):
        self.nt = int(nt)
        self.time = time
        self.time_sum_path = time_sum_path
        for name in SET_NAMES:
            res, zon = sets[name]
            setattr(self, name, ResultSet(owner, name, res, zon, time))


class Builder:
    """The device side, driven by ``TEMDiagnostics``: ``add`` every block of the four fields, ``run_stationary`` once
    all are in, ``finish`` with the gathered zonal intermediates of the ordinary run."""

    def __init__(self, owner, plan):
        self.owner, self.plan = owner, plan
        work = str(owner._work_dtype).replace("torch.", "")
        self.path = "kernel" if TIME_SUM_KERNEL[work] else "torch"
        self.acc = None
        self.nt = 0
        self.stat_flux = None

    def add(self, fields):
        """Time sum of one block ``[ncol][nlev][ntb]`` of ua va ta wap, on the current stream."""
        import torch
        fields = list(fields)
        if self.path == "kernel":
            self.acc = self.plan.time_sum(fields, acc=self.acc, accumulate=self.acc is not None)
        else:
            sums = [torch.sum(x, -1, dtype=torch.float64) for x in fields]
            if self.acc is None:
                self.acc = sums
            else:
                for a, s in zip(self.acc, sums):
                    a += s
        self.nt += int(fields[0].shape[-1])

    def run_stationary(self):
        """TEM of the time-mean fields (fp64 whatever the work dtype): the plan is left set for ``nt = 1``."""
        o, plan = self.owner, self.plan
        means = [(a / float(self.nt)).unsqueeze(-1).contiguous() for a in self.acc]
        self.acc = None
        plan.set_tem(o.NLEV, 1, o._p_np, float(o.p0))
        _, zon = plan.tem_run(*means, want_zonal=True)
        if plan.status():
            raise RuntimeError(_NAN_MESSAGE)
        i0 = _lib.ZONAL_NAMES.index(FLUX_NAMES[0])
        self.stat_flux = zon[i0:i0 + 3].clone()

    def finish(self, zon_all):
        """``zon_all``: ``[16][M][nlev][NT]`` of the ordinary run -> TEMClimatology."""
        total = zon_all[:7].mean(dim=-1, keepdim=True)          # mean state and total fluxes, [7][M][nlev][1]
        fluxes = {"total": total[4:7], "stationary": self.stat_flux, "transient": total[4:7] - self.stat_flux}
        sets = {}
        for name in SET_NAMES:
            zm7 = total.clone()
            zm7[4:7] = fluxes[name]
            sets[name] = self.plan.tem_from_zonal_means(zm7, want_zonal=True)
        return TEMClimatology(self.owner, sets, self.nt, mean_time(self.owner.time), self.path)
