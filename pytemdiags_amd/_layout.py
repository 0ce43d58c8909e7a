"""ctypes binding of the third header of libtemx.so, include/temx_layout.h (time-major records to engine layout).

Same shape as ``_vert``: one table of (name, restype, argtypes) for every symbol the header declares.  The library
is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

LAYOUT_VERSION = 100        # temxl_version() of the library these bindings were written for
NF_MAX = 8
FLIP_LEV = 1

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = [
    ("temxl_version", _i, []),
    ("temxl_to_engine", _i, [_i, _i, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_vp), _i, _i64, _i, _i64, _i64, _i64,
                             _i, _vp]),
]


def load():
    """libtemx.so with the temxl_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxl_version", LAYOUT_VERSION, "temx_layout")
