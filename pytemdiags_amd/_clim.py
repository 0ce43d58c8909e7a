"""ctypes binding of the fifth header of libtemx.so, include/temx_clim.h (time sums and the TEM epilogue on the caller's
zonal means: the device steps of a time-mean TEM).

Same shape as ``_layout``: one table of (name, restype, argtypes) for every symbol the header declares.  The library
is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

CLIM_VERSION = 100          # temxc_version() of the library these bindings were written for
NF_MAX = 8
ACCUMULATE = 1

# how csrc/clim_shapes.hpp cuts a launch of the time sum (tests/test_clim_host.py holds these to the header)
THREADS = 256
LDS_BYTES = 32 * 1024
MIN_ROWS = 16

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = [
    ("temxc_version", _i, []),
    ("temxc_time_sum", _i, [_i, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i64, _i, _i64, _i, _vp]),
    ("temxc_tem_from_zonal_means", _i, [_vp, _vp, _i64, _vp, _vp, _vp]),
]


def switch_nt(itemsize):
    """The smallest ``nt`` whose rows take the long-row kernel of the time sum, for sources of ``itemsize`` bytes per
    element (``clim_switch_nt`` of csrc/clim_shapes.hpp): a row is staged through LDS while at least ``MIN_ROWS`` rows
    of ``nt | 1`` elements fit ``LDS_BYTES``."""
    budget = LDS_BYTES // int(itemsize)
    nt = 1
    while (nt | 1) <= budget and budget // (nt | 1) >= MIN_ROWS:
        nt += 1
    return nt


def load():
    """libtemx.so with the temxc_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxc_version", CLIM_VERSION, "temx_clim")
