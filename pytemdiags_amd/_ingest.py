"""ctypes binding of the fourth header of libtemx.so, include/temx_ingest.h (time-major model-level records to
pressure levels in the engine's layout).

Same shape as ``_vert`` and ``_layout``: one table of (name, restype, argtypes) for every symbol the header declares.
The library is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h,
``method`` and ``edge`` take the values of ``_vert.METHODS`` / ``_vert.EDGES``.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

INGEST_VERSION = 100        # temxi_version() of the library these bindings were written for
NF_MAX = 8

_vp, _i, _i64, _d = C.c_void_p, C.c_int, C.c_int64, C.c_double
_dp = C.POINTER(C.c_double)
SIGNATURES = [
    ("temxi_version", _i, []),
    ("temxi_records_to_pressure", _i, [_i, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, _i64, _i, _i64, _i64,
                                       _i64, _i, _dp, _dp, _dp, _d, _vp, _i, _i, _i, _vp]),
]


def load():
    """libtemx.so with the temxi_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxi_version", INGEST_VERSION, "temx_ingest")
