"""ctypes binding of the twelfth header of libtemx.so, pytemdiags_amd/include_wavecls/temx_wavecls.h (the class form of the
zonal-wavenumber fit: the sums of the fit per latitude class instead of per column).

Same shape as ``_wave``: one table of (name, restype, argtypes) for every symbol the header declares.  The library is the
one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

WAVECLS_VERSION = 100       # temxz_version() of the library these bindings were written for
NF_MAX = 8
NM_MAX = 64
NDEG_MAX = 64

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = [
    ("temxz_version", _i, []),
    ("temxz_wave_create", _i, [C.POINTER(_vp), _vp, C.POINTER(C.c_double), _i, C.POINTER(_i)]),
    ("temxz_wave_destroy", None, [_vp]),
    ("temxz_wave_workspace_bytes", _i64, [_vp]),
    ("temxz_wave_project", _i, [_vp, _i, _i, C.POINTER(_vp), C.POINTER(_i), _i64, _vp, _vp, _vp]),
    ("temxz_wave_fluxes", _i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    ("temxz_wave_status", _i, [_vp, C.POINTER(_i), _vp]),
    ("temxz_wave_shape", _i, [_i, _i, C.POINTER(_i)]),
    ("temxz_wave_launch", _i, [_vp, _i, _i, _i64, C.POINTER(_i)]),
]


def shape(L, m):
    """``wavecls_shape`` of csrc/wave_class_tables.hpp as a dict (``temxz_wave_shape``): ndeg, Kc, TBS (blocks of four
    degrees per parity of l - m), nacc (accumulators per field and lane), fpw (fields per wave)."""
    out = (C.c_int * 5)()
    check(load().temxz_wave_shape(int(L), int(m), out))
    return dict(zip(("ndeg", "Kc", "TBS", "nacc", "fpw"), (int(v) for v in out)))


def launch(handle, mi, nf, D):
    """How the sweep of ``nf`` (4: the fluxes, 1: a projection) fields of ``D`` columns on wavenumber ``mi`` of the state
    is cut (``temxz_wave_launch``): TBS, ndt (d-tiles), pieces, inside (cuts that fall inside a class-group)."""
    out = (C.c_int * 4)()
    check(load().temxz_wave_launch(handle, int(mi), int(nf), int(D), out))
    return dict(zip(("TBS", "ndt", "pieces", "inside"), (int(v) for v in out)))


def load():
    """libtemx.so with the temxz_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxz_version", WAVECLS_VERSION, "temx_wavecls")
