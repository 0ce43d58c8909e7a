"""ctypes binding of the tenth header of libtemx.so, pytemdiags_amd/include/temx_wave.h (zonal wavenumbers on an
unstructured grid: the wave-m component of a field and the wave-m eddy fluxes on the zonal grid).

Same shape as ``_gclim``: one table of (name, restype, argtypes) for every symbol the header declares.  The library
is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

WAVE_VERSION = 100          # temxk_version() of the library these bindings were written for
NF_MAX = 8
NM_MAX = 64
KC_MAX = 512

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = [
    ("temxk_version", _i, []),
    ("temxk_wave_create", _i, [C.POINTER(_vp), _vp, C.POINTER(C.c_double), _i, C.POINTER(_i)]),
    ("temxk_wave_destroy", None, [_vp]),
    ("temxk_wave_workspace_bytes", _i64, [_vp]),
    ("temxk_wave_project", _i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_i), _i64, _vp, _vp, _vp]),
    ("temxk_wave_fluxes", _i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    ("temxk_wave_status", _i, [_vp, C.POINTER(_i), _vp]),
    ("temxk_wave_shape", _i, [_i, _i, C.POINTER(_i)]),
    ("temxk_wave_timing", _i, [_vp, _i]),
    ("temxk_wave_timing_read", _i, [_vp, _vp, C.POINTER(_i)]),
]


def kc(L, m):
    """Basis columns of wavenumber ``m`` at truncation ``L`` (``wave_kc``): cos and sin of the degrees m..L."""
    return 2 * (int(L) + 1 - int(m))


def shape(L, m):
    """``wave_shape`` of csrc/wave_tables.hpp as a dict (``temxk_wave_shape``): ndeg, Kc, nslice, tb_last, gstride, kpad."""
    out = (C.c_int * 6)()
    check(load().temxk_wave_shape(int(L), int(m), out))
    return dict(zip(("ndeg", "Kc", "nslice", "tb_last", "gstride", "kpad"), (int(v) for v in out)))


def load():
    """libtemx.so with the temxk_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxk_version", WAVE_VERSION, "temx_wave")
