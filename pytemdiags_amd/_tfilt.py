"""ctypes binding of the eleventh header of libtemx.so, pytemdiags_amd/include/temx_tfilt.h (a finite-impulse-response
filter along the time axis of fields in the engine's layout: the device step of the EP flux by time scale).

Same shape as ``_wave``: one table of (name, restype, argtypes) for every symbol the header declares.  The library is the
one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

TFILT_VERSION = 100         # temxf_version() of the library these bindings were written for
NF_MAX = 8
NB_MAX = 4
NW_MAX = 255
SHAPE_NAMES = ("rpb", "TT", "stride", "R", "ntile", "grid", "lds_bytes")

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = [
    ("temxf_version", _i, []),
    ("temxf_filter_time", _i, [_i, _i, C.POINTER(_vp), C.POINTER(_i), _i, C.POINTER(_vp), _i, _i64, _i, _i64, _i,
                               _vp, _i, _vp]),
    ("temxf_filter_shape", _i, [_i64, _i64, _i, _i, _i, _i, C.POINTER(_i)]),
]


def shape(rows, nt, nw, nb=1, src_esz=8, dst_esz=8):
    """``tfilt_shape`` of csrc/tfilt_shapes.hpp as a dict (``temxf_filter_shape``): rpb, TT, stride, R, ntile, grid,
    lds_bytes."""
    out = (C.c_int * len(SHAPE_NAMES))()
    check(load().temxf_filter_shape(int(rows), int(nt), int(nw), int(nb), int(src_esz), int(dst_esz), out))
    return dict(zip(SHAPE_NAMES, (int(v) for v in out)))


def load():
    """libtemx.so with the temxf_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxf_version", TFILT_VERSION, "temx_tfilt")
