"""Time-major records, host side: the block list, the time-major test, the argument checks that must fail before any
device call, the ctypes table against include/temx_layout.h and the plain-C link check.  Needs no GPU."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA_DIMS = ("ncol", "plev", "time")


# ---- time_blocks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,tb", [(11, 4), (12, 4), (11, 11), (11, 16), (1, 1), (1, 5), (7, 1), (730, 32)])
def test_time_blocks_cover_every_snapshot_once_short_block_last(nt, tb):
    from pytemdiags_amd.layout import time_blocks
    blocks = time_blocks(nt, tb)
    assert blocks[0][0] == 0 and blocks[-1][1] == nt
    assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))            # in order, no gap, no overlap
    seen = np.zeros(nt, dtype=int)
    for t0, t1 in blocks:
        assert 0 <= t0 < t1 <= nt
        seen[t0:t1] += 1
    assert np.all(seen == 1)
    sizes = [t1 - t0 for t0, t1 in blocks]
    assert all(s == min(tb, nt) for s in sizes[:-1]) and 1 <= sizes[-1] <= min(tb, nt)
    assert len(set(sizes)) <= 2                                             # set_tem is called again at most once
    assert len(blocks) == -(-nt // tb)


def test_time_blocks_refuses_empty():
    from pytemdiags_amd.layout import time_blocks
    with pytest.raises(ValueError):
        time_blocks(0, 4)
    with pytest.raises(ValueError):
        time_blocks(4, 0)


# ---- is_time_major -----------------------------------------------------------------------------------------------
def test_is_time_major_dims_orders_views_and_2d():
    import itertools
    import torch
    from pytemdiags_amd.layout import is_time_major
    a = np.zeros((5, 3, 7))
    for dims in itertools.permutations(DATA_DIMS):
        assert is_time_major(dims, DATA_DIMS, a) == (dims == ("time", "plev", "ncol")), dims
    tm = ("time", "plev", "ncol")
    assert is_time_major(tm, DATA_DIMS, torch.zeros(5, 3, 7))
    assert is_time_major(list(tm), DATA_DIMS, a)
    # other names for the three axes
    assert is_time_major(("t", "lev", "col"), ("col", "lev", "t"), a)
    assert not is_time_major(("t", "lev", "col"), DATA_DIMS, a)
    # views that are not C-contiguous
    assert not is_time_major(tm, DATA_DIMS, a[:, :, ::2])
    assert not is_time_major(tm, DATA_DIMS, np.zeros((7, 3, 5)).transpose(2, 1, 0))
    assert not is_time_major(tm, DATA_DIMS, np.asfortranarray(a))
    assert not is_time_major(tm, DATA_DIMS, torch.zeros(7, 3, 5).permute(2, 1, 0))
    assert is_time_major(tm, DATA_DIMS, a[1:4])                              # a time block of it still is
    # 2-D input is never time-major
    assert not is_time_major(("plev", "ncol"), DATA_DIMS, np.zeros((3, 7)))
    assert not is_time_major(("time", "ncol"), DATA_DIMS, np.zeros((3, 7)))
    assert not is_time_major(tm, DATA_DIMS, np.zeros((3, 7)))


def test_is_time_major_memmap(tmp_path):
    from pytemdiags_amd.layout import is_time_major
    m = np.memmap(str(tmp_path / "rec.bin"), dtype=np.float32, mode="w+", shape=(4, 3, 6))
    assert is_time_major(("time", "plev", "ncol"), DATA_DIMS, m)
    assert not is_time_major(("ncol", "plev", "time"), DATA_DIMS, m)


# ---- time_block validation before any device call -------------------------------------------------------------------
def _tiny():
    la = -90 + (np.arange(6) + 0.5) * 30.0
    lat = np.repeat(la, 8)
    plev = np.array([100.0, 500.0, 1000.0])
    f = np.zeros((lat.size, 3, 2))
    return lat, plev, f


@pytest.mark.parametrize("bad", [0, -3, 2.0, 2.5, "4", True, (4,)])
def test_temdiagnostics_rejects_bad_time_block_before_device(bad):
    from pytemdiags_amd import TEMDiagnostics
    lat, plev, f = _tiny()
    with pytest.raises(ValueError, match="time_block"):
        TEMDiagnostics(f, f, f, f, lat, plev=plev, time_block=bad)


def test_time_block_is_keyword_only():
    import inspect
    from pytemdiags_amd import TEMDiagnostics
    p = inspect.signature(TEMDiagnostics.__init__).parameters["time_block"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_check_time_block_accepts_integers():
    from pytemdiags_amd.layout import check_time_block
    assert check_time_block(None) is None
    assert check_time_block(1) == 1 and check_time_block(np.int64(16)) == 16
    assert isinstance(check_time_block(np.int32(3)), int)


# ---- the ctypes table against the header ------------------------------------------------------------------------------
def test_layout_header_declares_exactly_what_is_bound():
    import ctypes as C
    from pytemdiags_amd import _layout, _lib
    hdr = open(os.path.join(ROOT, "include", "temx_layout.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(temxl_[a-z0-9_]+)\s*\(", code))
    assert declared == {n for n, _, _ in _layout.SIGNATURES} == {"temxl_version", "temxl_to_engine"}
    assert not re.findall(r"\b(temxv?_[a-z0-9_]+)\s*\(", code)      # the other headers' ABI is not extended from here
    lib = _layout.load()
    assert lib is _lib.load() and lib.temxl_version() == _layout.LAYOUT_VERSION == 100
    for name, value in (("TEMXL_NF_MAX", _layout.NF_MAX), ("TEMXL_FLIP_LEV", _layout.FLIP_LEV)):
        assert re.search(r"\b%s = %d\b" % (name, value), code), name
    # the declared parameter list, type by type, against the argtypes
    decl = re.search(r"int temxl_to_engine\((.*?)\);", code, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "void*": C.c_void_p, "const void* const*": C.POINTER(C.c_void_p),
             "void* const*": C.POINTER(C.c_void_p), "const int*": C.POINTER(C.c_int)}
    want = [ctype[p.rsplit(" ", 1)[0]] for p in params]
    sig = dict((n, (r, a)) for n, r, a in _layout.SIGNATURES)
    assert sig["temxl_to_engine"] == (C.c_int, want)
    assert sig["temxl_version"] == (C.c_int, [])
    assert [p.rsplit(" ", 1)[1] for p in params] == [
        "device", "nf", "src_host", "src_dtype_host", "dst_host", "dst_dtype", "ncol", "nlev", "nt_src", "t0", "ntb",
        "flags", "stream"]
    # the entry point with a body is a function-try-block, like every other one; the other versions stand
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    assert re.search(r"^int temxl_to_engine\([^;{]*\)\s*try \{\s*$", src, re.M)
    assert "int temx_version(void) { return 402; }" in src and "int temxv_version(void) { return 100; }" in src


def test_whole_run_gate_is_backed_by_a_committed_measurement():
    """``layout.WHOLE_RUN_KERNEL`` may switch the kernel on for a dtype only if profiles/relayout_bench_mi355x.json
    shows it no slower than the torch copy in every leg that writes that dtype, at the three shapes."""
    import json
    from pytemdiags_amd import layout
    assert set(layout.WHOLE_RUN_KERNEL) == {"float64", "float32"}
    path = os.path.join(ROOT, "profiles", "relayout_bench_mi355x.json")
    for name, on in layout.WHOLE_RUN_KERNEL.items():
        if not on:
            continue
        assert os.path.exists(path), "WHOLE_RUN_KERNEL[%r] is on without a measurement" % name
        legs = [r for r in json.load(open(path))["legs"] if r.get("dst_dtype") == name]
        shapes = {(r["ncol"], r["nlev"], r["nt"]) for r in legs}
        assert {(777602, 72, 30)} <= shapes and (name == "float32" or (48602, 72, 92) in shapes)
        assert all(r["equal_to_torch"] and r["torch_over_relayout_time"] >= 1.0 for r in legs), name


def test_layout_argument_checks_come_before_any_device_call():
    import ctypes as C
    from pytemdiags_amd import _layout
    lib = _layout.load()
    src, dst = (C.c_void_p * 1)(4096), (C.c_void_p * 1)(1 << 20)
    f64 = (C.c_int * 1)(0)

    def call(nf=1, src=src, sdt=f64, dst=dst, ddt=0, ncol=4, nlev=3, nt_src=5, t0=1, ntb=2, flags=0):
        # device 99 does not exist: a call that got as far as the device would come back TEMX_EHIP, not TEMX_EINVAL
        return lib.temxl_to_engine(99, nf, src, sdt, dst, ddt, ncol, nlev, nt_src, t0, ntb, flags, None)
    assert call(nf=0) == -1 and b"nf" in lib.temx_last_error()
    assert call(nf=9) == -1
    assert call(src=None) == -1 and call(dst=None) == -1 and call(sdt=None) == -1
    assert call(t0=4) == -1 and b"nt_src" in lib.temx_last_error()
    assert call(sdt=(C.c_int * 1)(0), ddt=1) == -1                 # fp64 -> fp32 narrows
    assert call(nlev=1) == -2                                      # well-formed, one level: only now is the device touched
    assert call() == -2


def test_layout_header_is_plain_c_and_links(tmp_path):
    from pytemdiags_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "link_check_layout")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "link_check_layout.c"), "-o", exe,
                    "-L", libdir, "-ltemx", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "temxl_version=100 nf0_rc=-1" in out.stdout
