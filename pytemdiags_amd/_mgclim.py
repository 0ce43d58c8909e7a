"""ctypes binding of the ninth header of libtemx.so, pytemdiags_amd/include/temx_mgclim.h (the grouped, weighted sum
over the valid times of fields with missing values: the device step of masked monthly, seasonal and weighted TEM
climatologies).

Same shape as ``_gclim``: one table of (name, restype, argtypes) for every symbol the header declares.  The library
is the one ``_lib.load()`` loads; error codes and ``temx_last_error()`` are those of include/temx.h.
"""
from __future__ import annotations

import ctypes as C

from . import _gclim, _lib, _nclim
from ._lib import F32, F64, TemxError, check  # noqa: F401  (re-exported for callers of this table)

MGCLIM_VERSION = 100        # temxw_version() of the library these bindings were written for
NF_MAX = 8
NG_MAX = 64
ACCUMULATE = 1
COMMON_MASK = 2

# how csrc/mgclim_shapes.hpp cuts a launch (tests/test_mgclim_host.py holds these to the header)
THREADS = 256
LDS_BYTES = _nclim.LDS_BYTES      # all staged images of a workgroup
LONG_LDS_BYTES = 64 * 1024        # LDS form of the long rows: the images of a workgroup's waves
LONG_ROWS = THREADS // 64
BOUNDS = _gclim.BOUNDS            # the long-row form by the groups present: registers for <= 1 and <= 4, LDS beyond

_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = [
    ("temxw_version", _i, []),
    ("temxw_time_sum_groups_valid", _i, [_i, _i, C.POINTER(_vp), _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _i64, _i,
                                         _i64, _i64, _i64, _i, C.POINTER(C.c_int32), C.POINTER(C.c_double), _i, _vp]),
]


def staged_fields(nf, common):
    """The fields a workgroup holds together: all ``nf`` under a common mask, one in own-mask mode."""
    return int(nf) if common else 1


def switch_nt(itemsize, nf=1, common=False):
    """The smallest ``nt`` whose rows take a long-row form (``mgclim_switch_nt``).  The order of the additions is that
    of the grouped sum, whose rows are cut by ``nt`` and the element size alone, so the switch is ``_gclim.switch_nt``
    whatever ``nf`` and the mask mode: below it the rows are staged, however few of them fit."""
    return _gclim.switch_nt(itemsize)


def bound(npresent):
    """The long-row form for ``npresent`` groups present in a block (``gclim_bound``): 1 or 4 registers, 64 LDS."""
    return _gclim.bound(npresent)


def batch(nfs):
    """Groups present that one walk of a long row takes in the LDS form (``mgclim_batch``): the slots of ``nfs + 2``
    outputs times 64 lanes that fit ``LONG_LDS_BYTES``."""
    return LONG_LDS_BYTES // ((int(nfs) + 2) * 512)


def shape(rows, nt, itemsize, nfs, npresent):
    """``mgclim_shape`` of csrc/mgclim_shapes.hpp as a dict: staged, rpb, stride, bound, batch, npass, rpw, nblk,
    lds_bytes."""
    rows, nt, nfs, npresent = int(rows), int(nt), int(nfs), int(npresent)
    s = dict(staged=0, rpb=0, stride=0, bound=0, batch=0, npass=1, rpw=0, lds_bytes=0)
    if nt < switch_nt(itemsize):
        n = _nclim.shape(rows, nt, itemsize, nfs)
        rpb = n["rpb"] if n["staged"] else _nclim.fit(nt, itemsize, nfs)
        s.update(staged=1, rpb=rpb, stride=nt | 1, rpw=rpb, lds_bytes=nfs * rpb * (nt | 1) * int(itemsize))
    else:
        s["bound"] = bound(npresent)
        if s["bound"] == BOUNDS[-1]:
            b = min(npresent, batch(nfs))
            fit = LONG_LDS_BYTES // (b * (nfs + 2) * 512)
            rpw = max(1, min(fit, LONG_ROWS))
            s.update(batch=b, npass=(npresent + b - 1) // b, rpw=rpw, lds_bytes=rpw * b * (nfs + 2) * 512)
        else:
            s["rpw"] = LONG_ROWS
    s["nblk"] = (rows + s["rpw"] - 1) // s["rpw"]
    return s


def load():
    """libtemx.so with the temxw_* entry points bound (once)."""
    return _lib.bind(SIGNATURES, "temxw_version", MGCLIM_VERSION, "temx_mgclim")
