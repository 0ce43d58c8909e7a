"""ctypes binding of the second header of libtemx.so, include/temx_vert.h (vertical interpolation).

Same shape as ``_lib``: one table of (name, restype, argtypes) for every symbol the header declares.  The library
is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

VERT_VERSION = 100          # temxv_version() of the library these bindings were written for
P_HYBRID, P_FIELD = 0, 1
LOG, LINEAR = 0, 1
EDGE_NAN, EDGE_HOLD = 0, 1
NF_MAX = 8
METHODS = {"log": LOG, "linear": LINEAR}
EDGES = {"nan": EDGE_NAN, "hold": EDGE_HOLD}

_vp, _i, _i64, _dp = C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_double)
SIGNATURES = [
    ("temxv_version", _i, []),
    ("temxv_interp", _i, [_i, _i, C.POINTER(_vp), C.POINTER(_vp), _i, _i64, _i, _i64, _i, _dp, _i, _dp, _dp,
                          C.c_double, _vp, _i, _i, _i, _vp]),
]


def load():
    """libtemx.so with the temxv_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxv_version", VERT_VERSION, "temx_vert")
