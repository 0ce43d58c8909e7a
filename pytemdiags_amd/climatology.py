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

Fields with missing values (``climatology=True, missing="mask", min_time_coverage=v``, ``0 < v <= 1``).  The mask of
real pressure-level data varies in time (surface pressure moves), so the time mean needs a contract of its own.  With
``need = max(1, ceil(v NT - 1e-9))``:

  * time-mean fields   per (column, level), each of the four fields is the sum over the times valid under the common
    mask of the four (as the masked TEM run defines it) divided by their count, and missing (NaN) where the count is
    below ``need``.  Sums and counts come from ``engine.Plan.time_sum_valid(common=True)``, fused into the block loop;
    they accumulate across blocks under ``time_block=``.  Division and thresholding are torch on ``[ncol][nlev]``.
  * stationary fluxes  ``upvpb upwappb vptpb`` of one masked TEM run (``nt = 1``) on those fp64 mean fields, under the
    object's ``min_coverage``; its zonal coverage is ``tem.climatology.stationary_coverage``.
  * mean state and total fluxes   per (lat, level) of the zonal grid, the mean over the snapshots whose per-snapshot
    masked zonal means are finite, NaN where fewer than ``need`` are.  The seven zonal means share their NaN pattern,
    so this is one ``time_sum_valid(common=False)`` call on the seven viewed as ``[7 M nlev rows][NT]``; the valid
    fraction is ``tem.climatology.time_coverage``, shape ``(lat, plev, 1)``.
  * transient fluxes   total - stationary.  Under a mask that varies in time this is a DEFINITION, not the identity it
    is without missing values: the mean state averages per-snapshot masked fits over the snapshots that have one, the
    stationary run fits the time-mean fields once, and the two no longer commute.
  * the three sets share the mean state; each is the epilogue of that state and its fluxes, and NaN propagates through
    the epilogue as it does in a masked run.

The ordinary masked run goes last: per-snapshot results, ``coverage``, native attributes and the plan's state are bit
for bit those of the same object built without ``climatology``.  No tracers, no ``lat_bins``; grouped means of masked
fields have a keyword of their own (``min_group_coverage``, below).

Grouped and weighted means (``climatology=True, time_groups=g, time_weights=w``).  ``[.]_g`` is the weighted mean over
the times labelled ``g``: ``sum_t w_t x_t / W_g`` with ``W_g = sum_t w_t`` over the group; a time labelled -1 is in no
group.  Everything above holds per group: the group means of a field are ``[ncol][nlev][G]``, the engine's layout with
``nt = G``, so the stationary part of all groups is ONE ordinary TEM run, the mean state and total fluxes are the
grouped means of the per-snapshot zonal means, transient = total - stationary per group, and the three sets come out of
three epilogues at ``nts = G`` with shape ``(lat, plev, G)``.  The device step is ``engine.Plan.time_sum_groups``
(temxg_time_sum_groups), fused into the block loop with the block's ``t0`` and accumulating from the second block on;
``GROUP_SUM_KERNEL`` chooses between it and ``torch.matmul`` with the ``[NT][G]`` weight matrix.  Not served: tracer
terms, the sharded runners, NetCDF output, more than 64 groups.

Masked grouped means (``climatology=True, missing="mask", min_group_coverage=v`` next to ``time_groups=`` and / or
``time_weights=``; ``0 < v <= 1``).  The two contracts above, per group.  With ``n_g`` the times labelled ``g`` (whatever
their weight) and ``need_g = max(1, ceil(v n_g - 1e-9))``:

  * group-mean fields  per (column, level, group), the weighted sum over the times of the group that are valid under
    the common mask of the four fields, divided by the sum of their weights: NaN where fewer than ``need_g`` of them
    are valid or their weights sum to zero.  The threshold goes by the count, which is exact; the division by the
    weight.  Sums, weight sums and counts come from ``engine.Plan.time_sum_groups_valid(common=True)``
    (temxw_time_sum_groups_valid), fused into the block loop at the block's ``t0`` and accumulating from the second
    block on; division and thresholding are torch on ``[ncol][nlev][G]``.
  * stationary fluxes  of ONE masked TEM run at ``nt = G`` on those fp64 mean fields under the object's
    ``min_coverage``; its zonal coverage is ``tem.climatology.stationary_coverage``, ``(lat, plev, G)``.
  * mean state and total fluxes   one ``time_sum_groups_valid(common=False)`` call on the seven per-snapshot masked
    zonal means viewed as ``[7 M nlev rows][NT]``, the same threshold rule; ``time_coverage`` is the count over
    ``n_g``, a true division, ``(lat, plev, G)``.
  * transient = total - stationary per group (a definition, as in the masked climatology); three epilogues at
    ``nts = G``.
``time_weights`` alone gives one weighted masked group.  ``min_time_coverage`` belongs to the ungrouped masked mean and
is refused next to ``min_group_coverage``.  No tracers, no ``lat_bins``, no ``ncol`` sharding.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib

# Whether the time sum of fields of a work dtype goes through the HIP kernel (temxc_time_sum) or through
# torch.sum(x, -1, dtype=float64).  Set from tools/clim_bench.py (profiles/clim_bench_mi355x.json): the kernel is on
# for a dtype where it is faster than torch at ne120 x 72 x 30.  The engine method is always the kernel.
TIME_SUM_KERNEL = {"float64": True, "float32": True}

# The same for the grouped sum of ``time_groups=`` / ``time_weights=`` (temxg_time_sum_groups against torch.matmul with
# the [NT][G] weight matrix, after ``.double()`` for fp32 fields).  Set from tools/gclim_bench.py
# (profiles/gclim_bench_mi355x.json): on for a dtype where the kernel is faster at ne120 x 72 x 30, two groups of 15.
GROUP_SUM_KERNEL = {"float64": True, "float32": True}
NG_MAX = 64

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


def check_flag(climatology, missing, min_time_coverage=None, min_group_coverage=None):
    """``climatology`` as a bool; ValueError for anything else, next to ``missing="mask"`` unless ``min_time_coverage``
    opts into the masked contract (or ``min_group_coverage``, which ``check_group_coverage`` has seen, into the masked
    grouped one), and for a ``min_time_coverage`` without both or outside (0, 1] (no device needed)."""
    if not isinstance(climatology, (bool, np.bool_)):
        raise ValueError("climatology must be True or False, got %r" % (climatology,))
    if min_group_coverage is not None and min_time_coverage is None:
        return bool(climatology)
    if min_time_coverage is not None:
        if not (climatology and missing == "mask"):
            raise ValueError("min_time_coverage belongs to the masked climatology: it needs climatology=True and "
                             "missing='mask'")
        time_coverage_value(min_time_coverage)
    elif climatology and missing == "mask":
        raise ValueError("climatology=True and missing='mask' exclude each other: a time mean over a mask that varies "
                         "in time needs a contract of its own")
    return bool(climatology)


def time_coverage_value(min_time_coverage):
    """``min_time_coverage`` as a float in (0, 1]; ValueError for anything else."""
    v = min_time_coverage
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 < float(v) <= 1.0:
        raise ValueError("min_time_coverage must be a number in (0, 1], got %r" % (v,))
    return float(v)


def check_group_coverage(min_group_coverage, climatology, missing, time_groups, time_weights, min_time_coverage=None):
    """``min_group_coverage`` as a float in (0, 1], or None when it is not given.  ValueError for a value that is no
    number in (0, 1], without ``climatology=True`` and ``missing="mask"``, without ``time_groups`` / ``time_weights``,
    and next to ``min_time_coverage`` (no device needed)."""
    v = min_group_coverage
    if v is None:
        return None
    if not isinstance(climatology, (bool, np.bool_)):
        raise ValueError("climatology must be True or False, got %r" % (climatology,))
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 < float(v) <= 1.0:
        raise ValueError("min_group_coverage must be a number in (0, 1], got %r" % (v,))
    if not (climatology and missing == "mask"):
        raise ValueError("min_group_coverage belongs to the masked grouped means: it needs climatology=True and "
                         "missing='mask'")
    if time_groups is None and time_weights is None:
        raise ValueError("min_group_coverage belongs to the masked grouped means: it needs time_groups= and/or "
                         "time_weights= (min_time_coverage serves the ungrouped masked mean)")
    if min_time_coverage is not None:
        raise ValueError("min_group_coverage and min_time_coverage exclude each other: the first is the threshold of "
                         "the masked grouped means, the second that of the ungrouped masked mean")
    return float(v)


def group_times_needed(min_group_coverage, counts):
    """``need_g = max(1, ceil(v n_g - 1e-9))`` per group, with ``n_g`` the times labelled g whatever their weight."""
    return np.array([times_needed(min_group_coverage, n) for n in counts], dtype=np.float64)


def times_needed(min_time_coverage, nt):
    """``need = max(1, ceil(v NT - 1e-9))``: the valid times a point of the masked climatology needs."""
    return max(1, int(math.ceil(float(min_time_coverage) * int(nt) - 1e-9)))


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


_MONTHS = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")
_SEASONS = ("DJF", "MAM", "JJA", "SON")


def calendar_groups(time, by):
    """Labels of a ``datetime64`` time axis by ``"month"``, ``"season"`` (DJF MAM JJA SON) or ``"year"`` ->
    (int32 labels, the groups' names).  The groups are the keys present, in calendar order (years ascending); December
    and the January after it both lie in DJF.  Pure numpy; ValueError for anything else."""
    if by not in ("month", "season", "year"):
        raise ValueError("time_groups must be 'month', 'season' or 'year' (or a sequence of labels), got %r" % (by,))
    t = None if time is None else np.asarray(time)
    if t is None or t.dtype.kind != "M" or t.ndim != 1:
        raise ValueError("time_groups=%r needs a datetime64 time coordinate (time= for raw arrays)" % (by,))
    if np.any(np.isnat(t)):
        raise ValueError("time_groups=%r: the time coordinate holds NaT" % (by,))
    months = t.astype("datetime64[M]").astype(np.int64)          # months since 1970-01
    if by == "year":
        key = months // 12 + 1970
        names = None
    elif by == "month":
        key = months % 12
        names = _MONTHS
    else:
        key = ((months % 12 + 1) % 12) // 3
        names = _SEASONS
    present = np.unique(key)
    labels = np.searchsorted(present, key).astype(np.int32)
    return labels, [str(int(k)) if names is None else names[int(k)] for k in present]


def check_group_flags(time_groups, time_weights, climatology, missing, min_group_coverage=None):
    """The part of the refusals that needs no sizes: either keyword without ``climatology=True`` or next to
    ``missing="mask"`` (unless ``min_group_coverage``, which ``check_group_coverage`` has seen, opts into the masked
    grouped means).  -> None when neither keyword is given, else ``(time_groups, time_weights)``."""
    if time_groups is None and time_weights is None:
        return None
    if climatology is not True and not (isinstance(climatology, np.bool_) and bool(climatology)):
        raise ValueError("time_groups / time_weights belong to the time-mean TEM: they need climatology=True")
    if missing == "mask" and min_group_coverage is None:
        raise ValueError("time_groups / time_weights and missing='mask' exclude each other: masked grouped means are "
                         "not served (climatology.py)")
    return time_groups, time_weights


class Groups:
    """The resolved ``time_groups`` / ``time_weights`` of a record: ``labels`` (int32, -1 or 0..ng-1), ``weights``
    (float64 or None: ones), ``ng``, ``names``, ``counts`` (times per group), ``wsum`` (total weight per group) and
    ``time`` (the weighted mean time of each group)."""

    def __init__(self, labels, weights, names, time):
        self.labels, self.weights, self.names = labels, weights, names
        self.ng = len(names)
        w = np.ones(labels.size) if weights is None else weights
        keep = labels >= 0
        self.counts = np.bincount(labels[keep], minlength=self.ng).astype(np.int64)
        self.wsum = np.bincount(labels[keep], weights=w[keep], minlength=self.ng).astype(np.float64)
        if np.any(self.wsum <= 0):
            raise ValueError("time_groups: group %d has no weight (every group needs a positive total weight)"
                             % int(np.nonzero(self.wsum <= 0)[0][0]))
        self.time = group_times(time, labels, w, self.ng)

    def matrix(self):
        """``Wm[t][g] = w_t [label_t == g]``, float64 ``(NT, ng)``: the weight matrix of the torch composition."""
        w = np.ones(self.labels.size) if self.weights is None else self.weights
        m = np.zeros((self.labels.size, self.ng))
        keep = np.nonzero(self.labels >= 0)[0]
        m[keep, self.labels[keep]] = w[keep]
        return m


def group_times(time, labels, w, ng):
    """The weighted mean of a time coordinate per group (numbers, datetime64; anything else keeps the first entry of
    each group)."""
    t = np.asarray(time)
    idx = [np.nonzero(labels == g)[0] for g in range(ng)]
    if t.dtype.kind in "iuf":
        return np.array([np.sum(w[i] * t[i].astype(np.float64)) / np.sum(w[i]) for i in idx])
    if t.dtype.kind in "Mm":
        out = []
        for i in idx:
            d = (t[i] - t[i[0]])
            out.append(t[i[0]] + np.int64(np.rint(np.sum(w[i] * d.astype("int64")) / np.sum(w[i]))).astype(d.dtype))
        return np.array(out, dtype=t.dtype)
    return np.array([t[i[0]] for i in idx])


def resolve_groups(time_groups, time_weights, nt, time):
    """``time_groups`` / ``time_weights`` against a record of ``nt`` times with coordinate ``time`` -> ``Groups``.
    ValueError for a wrong length, a label out of range, more than ``NG_MAX`` groups, a group with no weight, a weight
    that is negative or not finite, and a calendar string without dates (no device needed)."""
    nt = int(nt)
    names = None
    if isinstance(time_groups, str):
        labels, names = calendar_groups(time, time_groups)
    elif time_groups is None:
        labels = np.zeros(nt, dtype=np.int32)
    else:
        g = np.asarray(time_groups)
        if g.ndim != 1 or g.dtype.kind not in "iu":
            raise ValueError("time_groups must be a one-dimensional integer sequence, 'month', 'season' or 'year'")
        if g.size and (g.min() < -1 or g.max() >= 2 ** 31):
            raise ValueError("time_groups: labels are -1 (left out) or 0..G-1, got %d" % (g.min() if g.min() < -1 else g.max()))
        labels = g.astype(np.int32)
    if labels.size != nt:
        raise ValueError("time_groups has %d entries but the record has %d times" % (labels.size, nt))
    ng = int(labels.max()) + 1 if labels.size else 0
    if ng < 1:
        raise ValueError("time_groups: no time belongs to a group")
    if ng > NG_MAX:
        raise ValueError("time_groups: %d groups, at most %d are served" % (ng, NG_MAX))
    weights = None
    if time_weights is not None:
        weights = np.array(time_weights, dtype=np.float64)
        if weights.ndim != 1 or weights.size != nt:
            raise ValueError("time_weights has shape %s but the record has %d times" % (weights.shape, nt))
        if not np.all(np.isfinite(weights)) or np.any(weights < 0):
            raise ValueError("time_weights must be finite and not negative")
    return Groups(labels, weights, list(range(ng)) if names is None else names, np.arange(nt) if time is None else time)


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
    snapshots averaged, ``time`` the mean of their time coordinate, ``time_sum_path`` ``"kernel"`` or ``"torch"``.
    Grouped means (``time_groups=`` / ``time_weights=``): the sets are ``(lat, plev, G)``, ``time`` holds the weighted
    mean time of each group, and ``groups`` (0..G-1), ``group_names`` (calendar names, else the integers),
    ``group_counts`` (times per group) and ``group_weights`` (total weight per group) describe them.
    Masked climatology: ``time_coverage`` is the fraction of the snapshots whose masked zonal means are finite and
    ``stationary_coverage`` the zonal coverage of the run on the time-mean fields, both ``(lat, plev, 1)`` float64 and
    labelled like ``ub``; None otherwise.  Masked grouped means: both are ``(lat, plev, G)``, ``time_coverage`` the
    fraction of each group's times."""

    def __init__(self, owner, sets, nt, time, time_sum_path, time_coverage=None, stationary_coverage=None, groups=None):
        self.nt = int(nt)
        self.time = time
        self.time_sum_path = time_sum_path
        if groups is not None:       # grouped means: the sets are (lat, plev, G), ``time`` the mean time of each group
            self.groups = np.arange(groups.ng)
            self.group_names = list(groups.names)
            self.group_counts = groups.counts.copy()
            self.group_weights = groups.wsum.copy()
        self._owner, self._tcov, self._scov = owner, time_coverage, stationary_coverage
        for name in SET_NAMES:
            res, zon = sets[name]
            setattr(self, name, ResultSet(owner, name, res, zon, time))


    def _coverage(self, t, name):
        return None if t is None else self._owner._wrap(t, name, "ua", force64=True, time=self.time)

    time_coverage = property(lambda s: s._coverage(s._tcov, "time_coverage"))
    stationary_coverage = property(lambda s: s._coverage(s._scov, "stationary_coverage"))


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


class MaskedBuilder(Builder):
    """The builder of a masked climatology (module docstring): the sums over valid times with their counts instead of
    the plain time sums, a masked stationary run, counted and thresholded means on the zonal grid."""

    def __init__(self, owner, plan, min_time_coverage):
        super().__init__(owner, plan)
        self.path = "kernel"
        self.v = time_coverage_value(min_time_coverage)
        self.cnt = None
        self.stat_cov = None

    def add(self, fields):
        fields = list(fields)
        first = self.acc is None
        self.acc, self.cnt = self.plan.time_sum_valid(fields, acc=self.acc, cnt=self.cnt, accumulate=not first, common=True)
        self.nt += int(fields[0].shape[-1])

    @staticmethod
    def _mean(acc, cnt, need):
        import torch
        nan = torch.full((), float("nan"), dtype=torch.float64, device=acc.device)
        return torch.where(cnt >= need, acc / cnt, nan)

    def run_stationary(self):
        o, plan = self.owner, self.plan
        need = times_needed(self.v, self.nt)
        means = [self._mean(a, self.cnt, need).unsqueeze(-1).contiguous() for a in self.acc]
        self.acc = self.cnt = None
        plan.set_tem(o.NLEV, 1, o._p_np, float(o.p0))
        _, zon = plan.tem_run(*means, want_zonal=True)
        self.stat_cov = plan.coverage().reshape(o.ZM_N, o.NLEV, 1)
        if plan.status():
            raise RuntimeError(_NAN_MESSAGE)
        i0 = _lib.ZONAL_NAMES.index(FLUX_NAMES[0])
        self.stat_flux = zon[i0:i0 + 3].clone()

    def finish(self, zon_all):
        """``zon_all``: ``[16][M][nlev][NT]`` of the ordinary masked run -> TEMClimatology."""
        _, M, nlev, nt = zon_all.shape
        need = times_needed(self.v, nt)
        (acc,), (cnt,) = self.plan.time_sum_valid([zon_all[:7].reshape(7 * M * nlev, 1, nt)], common=False)
        total = self._mean(acc, cnt, need).reshape(7, M, nlev, 1)
        import torch
        # (tensor by tensor: a true division, so that 3 of 5 is 0.6 and not 3 * 0.2)
        tcov = torch.true_divide(cnt.reshape(7, M, nlev, 1)[0], torch.full((), float(nt), dtype=torch.float64, device=cnt.device))
        fluxes = {"total": total[4:7], "stationary": self.stat_flux, "transient": total[4:7] - self.stat_flux}
        sets = {}
        for name in SET_NAMES:
            zm7 = total.clone()
            zm7[4:7] = fluxes[name]
            sets[name] = self.plan.tem_from_zonal_means(zm7, want_zonal=True)
        return TEMClimatology(self.owner, sets, self.nt, mean_time(self.owner.time), self.path, tcov, self.stat_cov)


class GroupedBuilder(Builder):
    """The builder of grouped and weighted means (module docstring): grouped sums at the block's ``t0`` instead of the
    plain time sums, one stationary run over all groups (``nt = G``), grouped means on the zonal grid."""

    def __init__(self, owner, plan, groups):
        super().__init__(owner, plan)
        work = str(owner._work_dtype).replace("torch.", "")
        self.path = "kernel" if GROUP_SUM_KERNEL[work] else "torch"
        self.groups = groups
        self.t0 = 0
        self._wm = None

    def _sums(self, fields, t0, acc):
        """Grouped sums of a block at ``t0`` -> list of fp64 ``[..][..][G]``; into ``acc`` (+=) when given."""
        import torch
        g = self.groups
        if self.path == "kernel":
            return self.plan.time_sum_groups(fields, g.labels, g.ng, g.weights, t0=t0, acc=acc, accumulate=acc is not None)
        if self._wm is None:
            self._wm = torch.as_tensor(g.matrix(), device=fields[0].device)
        wm = self._wm[t0:t0 + int(fields[0].shape[-1])]
        sums = [torch.matmul(x.double(), wm) for x in fields]
        if acc is None:
            return sums
        for a, s in zip(acc, sums):
            a += s
        return acc

    def add(self, fields):
        fields = list(fields)
        self.acc = self._sums(fields, self.t0, self.acc)
        self.t0 += int(fields[0].shape[-1])
        self.nt = self.t0

    def _wsum(self, like):
        import torch
        return torch.as_tensor(self.groups.wsum, device=like.device)

    def run_stationary(self):
        """TEM of the group-mean fields, all groups in one run (fp64 whatever the work dtype): the plan is left set for
        ``nt = G``."""
        o, plan, G = self.owner, self.plan, self.groups.ng
        means = [(a / self._wsum(a)).contiguous() for a in self.acc]
        self.acc = None
        plan.set_tem(o.NLEV, G, o._p_np, float(o.p0))
        _, zon = plan.tem_run(*means, want_zonal=True)
        if plan.status():
            raise RuntimeError(_NAN_MESSAGE)
        i0 = _lib.ZONAL_NAMES.index(FLUX_NAMES[0])
        self.stat_flux = zon[i0:i0 + 3].clone()

    def finish(self, zon_all):
        """``zon_all``: ``[16][M][nlev][NT]`` of the ordinary run -> TEMClimatology with sets ``(lat, plev, G)``."""
        _, M, nlev, nt = zon_all.shape
        G = self.groups.ng
        (acc,) = self._sums([zon_all[:7].reshape(7 * M * nlev, 1, nt)], 0, None)
        total = (acc / self._wsum(acc)).reshape(7, M, nlev, G)
        fluxes = {"total": total[4:7], "stationary": self.stat_flux, "transient": total[4:7] - self.stat_flux}
        sets = {}
        for name in SET_NAMES:
            zm7 = total.clone()
            zm7[4:7] = fluxes[name]
            sets[name] = self.plan.tem_from_zonal_means(zm7, want_zonal=True)
        return TEMClimatology(self.owner, sets, nt, self.groups.time, self.path, groups=self.groups)


class MaskedGroupedBuilder(Builder):
    """The builder of masked grouped means (module docstring): grouped sums over the valid times with their weight sums
    and counts at the block's ``t0``, one masked stationary run over all groups (``nt = G``), counted, weighted and
    thresholded group means on the zonal grid."""

    def __init__(self, owner, plan, groups, min_group_coverage):
        super().__init__(owner, plan)
        self.path = "kernel"
        self.groups = groups
        self.v = float(min_group_coverage)
        self.need = group_times_needed(self.v, groups.counts)
        self.t0 = 0
        self.wsum = self.cnt = None
        self.stat_cov = None

    def add(self, fields):
        fields = list(fields)
        g = self.groups
        first = self.acc is None
        self.acc, self.wsum, self.cnt = self.plan.time_sum_groups_valid(
            fields, g.labels, g.ng, g.weights, t0=self.t0, acc=self.acc, wsum=self.wsum, cnt=self.cnt, accumulate=not first,
            common=True)
        self.t0 += int(fields[0].shape[-1])
        self.nt = self.t0

    def _mean(self, acc, wsum, cnt):
        """``acc / wsum`` where at least ``need_g`` times are valid and carry weight, NaN elsewhere (``[..][G]``)."""
        import torch
        need = torch.as_tensor(self.need, device=acc.device)
        nan = torch.full((), float("nan"), dtype=torch.float64, device=acc.device)
        return torch.where((cnt >= need) & (wsum > 0), acc / wsum, nan)

    def run_stationary(self):
        """Masked TEM of the group-mean fields, all groups in one run (fp64 whatever the work dtype): the plan is left
        set for ``nt = G``."""
        o, plan, G = self.owner, self.plan, self.groups.ng
        means = [self._mean(a, self.wsum, self.cnt).contiguous() for a in self.acc]
        self.acc = self.wsum = self.cnt = None
        plan.set_tem(o.NLEV, G, o._p_np, float(o.p0))
        _, zon = plan.tem_run(*means, want_zonal=True)
        self.stat_cov = plan.coverage().reshape(o.ZM_N, o.NLEV, G)
        if plan.status():
            raise RuntimeError(_NAN_MESSAGE)
        i0 = _lib.ZONAL_NAMES.index(FLUX_NAMES[0])
        self.stat_flux = zon[i0:i0 + 3].clone()

    def finish(self, zon_all):
        """``zon_all``: ``[16][M][nlev][NT]`` of the ordinary masked run -> TEMClimatology with sets ``(lat, plev, G)``."""
        import torch
        _, M, nlev, nt = zon_all.shape
        g = self.groups
        G = g.ng
        (acc,), (wsum,), (cnt,) = self.plan.time_sum_groups_valid([zon_all[:7].reshape(7 * M * nlev, 1, nt)], g.labels, G,
                                                                  g.weights, common=False)
        total = self._mean(acc, wsum, cnt).reshape(7, M, nlev, G)
        # (tensor by tensor: a true division, so that 3 of 5 is 0.6 and not 3 * 0.2)
        tcov = torch.true_divide(cnt.reshape(7, M, nlev, G)[0], torch.as_tensor(g.counts.astype(np.float64), device=cnt.device))
        fluxes = {"total": total[4:7], "stationary": self.stat_flux, "transient": total[4:7] - self.stat_flux}
        sets = {}
        for name in SET_NAMES:
            zm7 = total.clone()
            zm7[4:7] = fluxes[name]
            sets[name] = self.plan.tem_from_zonal_means(zm7, want_zonal=True)
        return TEMClimatology(self.owner, sets, nt, g.time, self.path, tcov, self.stat_cov, groups=g)
