"""ctypes binding of the seventh header of libtemx.so, include/temx_nclim.h (the time sum over the valid times of
fields with missing values: the device step of a time-mean TEM in missing-value mode).

Same shape as ``_clim``: one table of (name, restype, argtypes) for every symbol the header declares.  The library
is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

NCLIM_VERSION = 100         # temxn_version() of the library these bindings were written for
NF_MAX = 8
ACCUMULATE = 1
COMMON_MASK = 2

# how csrc/nclim_shapes.hpp cuts a launch (tests/test_nclim_host.py holds these to the header)
THREADS = 256
LDS_BYTES = 32 * 1024
MIN_ROWS = 16
LONG_ROWS = THREADS // 64

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = [
    ("temxn_version", _i, []),
    ("temxn_time_sum_valid", _i, [_i, _i, C.POINTER(_vp), _i, C.POINTER(_vp), C.POINTER(_vp), _i64, _i, _i64, _i, _vp]),
]


def staged_fields(nf, common):
    """The fields a workgroup holds together: all ``nf`` under a common mask, one in own-mask mode."""
    return int(nf) if common else 1


def fit(nt, itemsize, nfs):
    """Rows of ``nt`` elements a workgroup can stage with ``nfs`` fields together (``nclim_fit``)."""
    budget = LDS_BYTES // int(itemsize) // int(nfs)
    stride = int(nt) | 1
    return budget // stride if stride <= budget else 0


def shape(rows, nt, itemsize, nfs):
    """``nclim_shape`` of csrc/nclim_shapes.hpp as a dict: staged, rpb, stride, g, nblk."""
    n = fit(nt, itemsize, nfs)
    if n >= MIN_ROWS:
        rpb = min(n, THREADS)
        g = 1
        while g < 64 and rpb * g * 2 <= THREADS:
            g *= 2
        s = dict(staged=1, rpb=rpb, stride=int(nt) | 1, g=g)
    else:
        s = dict(staged=0, rpb=LONG_ROWS, stride=0, g=64)
    s["nblk"] = (int(rows) + s["rpb"] - 1) // s["rpb"]
    return s


def switch_nt(itemsize, nf=1, common=False):
    """The smallest ``nt`` whose rows take the long-row kernel, for sources of ``itemsize`` bytes per element, ``nf``
    fields and the mask mode (``nclim_switch_nt``): a row is staged through LDS while at least ``MIN_ROWS`` rows of
    ``nt | 1`` elements of every field a workgroup holds fit ``LDS_BYTES``."""
    nfs = staged_fields(nf, common)
    nt = 1
    while fit(nt, itemsize, nfs) >= MIN_ROWS:
        nt += 1
    return nt


def load():
    """libtemx.so with the temxn_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxn_version", NCLIM_VERSION, "temx_nclim")
