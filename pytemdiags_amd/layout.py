"""Time-major records: GPU re-layout and the block sources of a blocked TEM run (include/temx_layout.h).

Model output arrives time-major, ``(time, lev, ncol)`` with ``ncol`` fastest; the engine works on
``[ncol][lev][time]`` with time fastest.  ``to_engine_layout`` moves a window of snapshots from the one to the other in
one kernel per eight fields (``temxl_to_engine``): each element read once and written once, the descending-``plev``
flip and the widening to the work dtype folded in.  A time block of a time-major array is one contiguous span, on the
host as on the device, which is what the block sources below build on.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _layout

# Whole runs (no time_block) of time-major input: does the kernel make the engine's copy, per work dtype?  The kernel
# replaces a torch copy there, so it is switched on for a dtype only by a measurement that shows it no slower than that
# copy at the three shapes of tools/relayout_bench.py, committed as profiles/relayout_bench_mi355x.json
# (tests/test_layout_host.py holds the two together).  Measured: 3.3 to 5.1 times faster than the torch copy in every
# leg, fp64 and fp32.  Blocked runs (time_block=) always use the kernel: there it replaces nothing.
WHOLE_RUN_KERNEL = {"float64": True, "float32": True}

# Largest piece a host field-block goes up in: the size of each of the two pinned staging buffers (bytes).
RING_CHUNK_BYTES = 256 << 20


def time_blocks(nt, time_block):
    """``[(t0, t1)]`` covering ``0 .. nt`` in order: full blocks of ``time_block`` first, the short remainder last."""
    nt, tb = int(nt), int(time_block)
    if nt < 1 or tb < 1:
        raise ValueError("time_blocks needs nt >= 1 and time_block >= 1, got %r, %r" % (nt, time_block))
    return [(t0, min(nt, t0 + tb)) for t0 in range(0, nt, tb)]


def check_time_block(time_block):
    """The ``time_block=`` argument of the front end: None, or an integer >= 1 (``ValueError`` otherwise)."""
    if time_block is None:
        return None
    if isinstance(time_block, bool) or not isinstance(time_block, (int, np.integer)):
        raise ValueError("time_block must be None or an integer >= 1, got %r" % (time_block,))
    if time_block < 1:
        raise ValueError("time_block must be at least 1, got %r" % (time_block,))
    return int(time_block)


def is_time_major(dims, data_dims, x):
    """True when ``x``, whose axes are named ``dims``, is a C-contiguous ``(time, vert, horz)`` array;
    ``data_dims`` names ``(horz, vert, time)``.  Host logic only: 2-D input is never time-major."""
    dims = tuple(dims)
    if len(dims) != 3 or getattr(x, "ndim", None) != 3:
        return False
    if dims != (data_dims[2], data_dims[1], data_dims[0]):
        return False
    if isinstance(x, np.ndarray):
        return bool(x.flags.c_contiguous)
    is_contiguous = getattr(x, "is_contiguous", None)
    return bool(is_contiguous()) if is_contiguous is not None else False


def to_engine_layout(srcs, t0=0, ntb=None, flip_lev=False, dtype=None, out=None):
    """Device tensors ``[nt][nlev][ncol]`` -> list of ``[ncol][nlev][ntb]`` tensors holding the snapshots
    ``t0 .. t0 + ntb`` (default: to the end), levels reversed under ``flip_lev``.

    ``srcs``: contiguous float64 / float32 tensors of one shape on one device (a single tensor is taken as a list of
    one).  ``dtype``: float32 when every source is float32, float64 otherwise; equal dtypes move bit for bit, float32
    widens to float64, float64 is never narrowed.  ``out``: tensors to write into instead of new ones.  The call is
    ordered on the current stream."""
    import torch
    lib = _layout.load()
    srcs = [srcs] if isinstance(srcs, torch.Tensor) else list(srcs)
    if not srcs:
        raise ValueError("no sources given")
    s0 = srcs[0]
    dts = {torch.float64: _layout.F64, torch.float32: _layout.F32}
    for s in srcs:
        if not (isinstance(s, torch.Tensor) and s.is_cuda and s.device == s0.device):
            raise ValueError("to_engine_layout needs device tensors on one device")
        if s.dim() != 3 or tuple(s.shape) != tuple(s0.shape) or not s.is_contiguous():
            raise ValueError("to_engine_layout needs contiguous [nt][nlev][ncol] tensors of one shape")
        if s.dtype not in dts:
            raise ValueError("to_engine_layout moves float64 and float32, got %s" % s.dtype)
    nt_src, nlev, ncol = (int(n) for n in s0.shape)
    t0 = int(t0)
    ntb = nt_src - t0 if ntb is None else int(ntb)
    if dtype is None:
        dtype = torch.float32 if all(s.dtype == torch.float32 for s in srcs) else torch.float64
    if dtype not in dts:
        raise ValueError("dtype must be float64 or float32, got %s" % (dtype,))
    if t0 < 0 or ntb < 1 or t0 + ntb > nt_src:
        raise ValueError("window t0 = %d, ntb = %d does not lie in 0 .. %d" % (t0, ntb, nt_src))
    with torch.cuda.device(s0.device):
        if out is None:            # one allocation for all fields
            out = torch.empty((len(srcs), ncol, nlev, ntb), dtype=dtype, device=s0.device).unbind(0)
        out = list(out)
        if len(out) != len(srcs):
            raise ValueError("out has %d tensors for %d sources" % (len(out), len(srcs)))
        for o in out:
            if not (o.is_cuda and o.device == s0.device and o.dtype == dtype and o.is_contiguous()
                    and tuple(o.shape) == (ncol, nlev, ntb)):
                raise ValueError("out needs contiguous %s tensors of shape %s on %s" % (dtype, (ncol, nlev, ntb), s0.device))
        stream = C.c_void_p(torch.cuda.current_stream(s0.device).cuda_stream)
        for g in range(0, len(srcs), _layout.NF_MAX):
            ss, oo = srcs[g:g + _layout.NF_MAX], out[g:g + _layout.NF_MAX]
            sp = (C.c_void_p * len(ss))(*[t.data_ptr() for t in ss])
            sd = (C.c_int * len(ss))(*[dts[t.dtype] for t in ss])
            op = (C.c_void_p * len(ss))(*[t.data_ptr() for t in oo])
            _layout.check(lib.temxl_to_engine(s0.device.index or 0, len(ss), sp, sd, op, dts[dtype], ncol, nlev, nt_src,
                                              t0, ntb, _layout.FLIP_LEV if flip_lev else 0, stream))
    return out


# ---- block sources: how one time block of all fields reaches engine layout -------------------------------------------
class DeviceBlocks:
    """Time-major device tensors: one ``to_engine_layout`` per block.  The device holds the source plus one block."""

    def __init__(self, srcs, flip_lev, work):
        self.srcs, self.flip, self.work = list(srcs), bool(flip_lev), work
        self._out = None
        self.timing = None

    def start(self, blocks):
        self.blocks = list(blocks)

    def get(self, n):
        t0, t1 = self.blocks[n]
        if self._out is not None and self._out[0].shape[2] != t1 - t0:
            self._out = None                      # the short last block: the full one is released first
        self._out = to_engine_layout(self.srcs, t0, t1 - t0, self.flip, self.work, out=self._out)
        return self._out

    def after_launch(self, n):
        pass

    def done(self, n):
        pass

    def close(self):
        self._out = None


class TorchBlocks:
    """Any other dims order: the block is sliced out of the ``[ncol][plev][time]`` views and made resident by torch,
    like a whole run."""

    def __init__(self, views, device, work):
        self.views, self.device, self.work = list(views), device, work
        self.timing = None

    def start(self, blocks):
        self.blocks = list(blocks)

    def get(self, n):
        t0, t1 = self.blocks[n]
        return [v[:, :, t0:t1].to(device=self.device, dtype=self.work).contiguous() for v in self.views]

    def after_launch(self, n):
        pass

    def done(self, n):
        pass

    def close(self):
        pass


class HostBlocks:
    """Time-major host arrays (``np.ndarray``, ``np.memmap``, CPU tensors).  A block of one field is one contiguous
    host span.  It goes up in consecutive byte chunks through a ring of two pinned buffers of at most
    ``RING_CHUNK_BYTES`` into one of two device upload buffers, on a copy stream; the compute stream waits for the
    block's event and re-lays it out.  Block n + 1 goes up while block n runs.  No host-side transpose and no
    whole-record tensor on either side.

    The arrays share the time axis and may differ in what follows it (``[nt][nlev_a][ncol]`` with a level count per
    array, or ``[nt][ncol]``): a slot holds a block of each in its own shape.  ``step(slot_tensors, ntb, out)`` is the
    work on the compute stream that turns the first ``ntb`` snapshots of a slot into the block's engine-layout
    tensors (default: the re-layout of all arrays); ``timing`` reports it under ``step_name``."""

    def __init__(self, arrays, device, flip_lev, work, step=None, step_name="relayout_ms"):
        import torch
        self.device, self.flip, self.work = device, bool(flip_lev), work
        self.step = step if step is not None else (
            lambda slot, ntb, out: to_engine_layout(slot, 0, ntb, self.flip, self.work, out=out))
        self.step_name = step_name
        self.host = []
        for a in arrays:
            a = a.numpy() if isinstance(a, torch.Tensor) else a
            self.host.append(a)
        self.tdt = [torch.float32 if a.dtype == np.float32 else torch.float64 for a in self.host]
        self.timing = {"upload_ms": [], step_name: [], "tem_ms": []}
        self._marks = []

    def start(self, blocks):
        import torch
        self.blocks = list(blocks)
        self.ntb_max = max(t1 - t0 for t0, t1 in self.blocks)
        pers = [self.ntb_max * int(np.prod(a.shape[1:])) for a in self.host]       # elements of a block, per array
        with torch.cuda.device(self.device):
            self.copy_stream = torch.cuda.Stream(self.device)
            # two upload slots, each one allocation: a time-major block of every field in its own dtype
            offs = np.concatenate([[0], np.cumsum([-(-per * a.dtype.itemsize // 512) * 512
                                                   for per, a in zip(pers, self.host)])])
            self.slots = []
            for _ in range(min(2, len(self.blocks))):
                raw = torch.empty(int(offs[-1]), dtype=torch.uint8, device=self.device)
                self.slots.append([raw[int(o):int(o) + per * a.dtype.itemsize].view(dt).view((self.ntb_max,) + tuple(a.shape[1:]))
                                   for o, per, a, dt in zip(offs, pers, self.host, self.tdt)])
        self.uploaded = [None] * len(self.slots)    # event: the slot's block has arrived
        self.consumed = [None] * len(self.slots)    # event: the slot's block has been re-laid out
        largest = max(per * a.dtype.itemsize for per, a in zip(pers, self.host))
        nring = max(1, min(int(RING_CHUNK_BYTES), largest))
        self.ring = [torch.empty(nring, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self.ring_np = [r.numpy() for r in self.ring]
        self.ring_free = [None, None]               # event: the H2D copy out of this pinned buffer has finished
        self._turn = 0
        self._out = None
        # the slots come from the caching allocator of the compute stream: work queued there may still read the memory
        self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        self._upload(0)

    def _upload(self, n):
        import torch
        t0, t1 = self.blocks[n]
        slot = n % len(self.slots)
        cs = self.copy_stream
        if self.consumed[slot] is not None:
            cs.wait_event(self.consumed[slot])
        ev0 = torch.cuda.Event(enable_timing=True)
        ev0.record(cs)
        for a, dst in zip(self.host, self.slots[slot]):
            span = a[t0:t1].reshape(-1).view(np.uint8)          # a view: the block of a time-major array is contiguous
            dbytes = dst.reshape(-1).view(torch.uint8)
            nring = self.ring_np[0].shape[0]
            for off in range(0, span.shape[0], nring):
                n_b = min(nring, span.shape[0] - off)
                i = self._turn
                self._turn ^= 1
                if self.ring_free[i] is not None:
                    self.ring_free[i].synchronize()
                self.ring_np[i][:n_b] = span[off:off + n_b]
                with torch.cuda.stream(cs):
                    dbytes[off:off + n_b].copy_(self.ring[i][:n_b], non_blocking=True)
                self.ring_free[i] = torch.cuda.Event()
                self.ring_free[i].record(cs)
        ev1 = torch.cuda.Event(enable_timing=True)
        ev1.record(cs)
        self.uploaded[slot] = ev1
        self._marks.append([ev0, ev1])

    def get(self, n):
        import torch
        t0, t1 = self.blocks[n]
        ntb = t1 - t0
        slot = n % len(self.slots)
        st = torch.cuda.current_stream(self.device)
        st.wait_event(self.uploaded[slot])
        if self._out is not None and self._out[0].shape[2] != ntb:
            self._out = None
        a = torch.cuda.Event(enable_timing=True)
        a.record(st)
        self._out = self.step(self.slots[slot], ntb, self._out)
        b = torch.cuda.Event(enable_timing=True)
        b.record(st)
        self.consumed[slot] = b
        self._marks[n] += [a, b]
        return self._out

    def after_launch(self, n):
        """Called once the TEM run of block n is queued: the next block goes up meanwhile."""
        if n + 1 < len(self.blocks):
            self._upload(n + 1)

    def done(self, n):
        """Called when everything of block n, tracer runs included, is queued: the end of its ``tem_ms``."""
        import torch
        c = torch.cuda.Event(enable_timing=True)
        c.record(torch.cuda.current_stream(self.device))
        self._marks[n].append(c)

    def close(self):
        """``timing``: per block, ``upload_ms`` on the copy stream, ``relayout_ms`` (the step) and ``tem_ms`` (TEM and tracer runs
        up to the gathering of the results) on the compute stream."""
        self.copy_stream.synchronize()
        for m in self._marks:
            if len(m) == 5:
                m[4].synchronize()
            if len(m) == 5:
                self.timing["upload_ms"].append(m[0].elapsed_time(m[1]))
                self.timing[self.step_name].append(m[2].elapsed_time(m[3]))
                self.timing["tem_ms"].append(m[3].elapsed_time(m[4]))
        self._out = self.slots = self.ring = self.ring_np = None
