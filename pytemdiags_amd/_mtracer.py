"""ctypes binding of the sixth header of libtemx.so, include/temx_mtracer.h (tracer TEM for fields with missing values:
the masked tracer run and its native fields).

Same shape as ``_clim``: one table of (name, restype, argtypes) for every symbol the header declares.  The library
is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import TemxError, check  # noqa: F401  (re-exported for callers of this table)

MTRACER_VERSION = 100       # temxm_version() of the library these bindings were written for

_vp, _i = C.c_void_p, C.c_int
SIGNATURES = [
    ("temxm_version", _i, []),
    ("temxm_tracer_run", _i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("temxm_tracer_eddy", _i, [_vp, _vp, _vp, _vp, _i, C.POINTER(_vp), _vp]),
]


def load():
    """libtemx.so with the temxm_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxm_version", MTRACER_VERSION, "temx_mtracer")
