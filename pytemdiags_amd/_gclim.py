"""ctypes binding of the eighth header of libtemx.so, include/temx_gclim.h (the grouped, weighted sum over time: the
device step of monthly, seasonal and yearly TEM climatologies and of weighted time means).

Same shape as ``_nclim``: one table of (name, restype, argtypes) for every symbol the header declares.  The library
is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _clim, _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

GCLIM_VERSION = 100         # temxg_version() of the library these bindings were written for
NF_MAX = 8
NG_MAX = 64
ACCUMULATE = 1

# the long-row kernel by the groups present in a block (csrc/dispatch.hpp): registers for at most 1 and at most 4, and
# accumulators in LDS beyond (64 stands for any number)
BOUNDS = (1, 4, 64)

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = [
    ("temxg_version", _i, []),
    ("temxg_time_sum_groups", _i, [_i, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i64, _i, _i64, _i64, _i64, _i,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_double), _i, _vp]),
]


def switch_nt(itemsize):
    """The smallest ``nt`` whose rows take the long-row kernel: the rows are cut as the plain time sum cuts them
    (``_clim.switch_nt``, ``clim_switch_nt`` of csrc/clim_shapes.hpp)."""
    return _clim.switch_nt(itemsize)


def bound(npresent):
    """The instantiation of the long-row kernel for ``npresent`` groups present in a block (``gclim_bound``)."""
    return next(b for b in BOUNDS if int(npresent) <= b)


def load():
    """libtemx.so with the temxg_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxg_version", GCLIM_VERSION, "temx_gclim")
