"""The argument rules of the four plan-free entry points (temxv_interp, temxl_to_engine, temxi_records_to_pressure,
temxc_time_sum), which pytemdiags_amd/csrc/field_args.hpp holds once: every refusal recorded before the rules moved out
of temx.hip (tests/golden/plan_free_refusals.json, written by tools/record_plan_free_refusals.py) replayed against the
library, the two refusals the move added on purpose, and the header on its own under AddressSanitizer + UBSan
(tests/host/field_args_main.cpp).  Needs no GPU: every call names device 99, so one that got past the checks comes
back TEMX_EHIP (-2)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_free_refusals.json")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
WORDS = ("nf", "null", "dtype", "pmode", "method", "edge", "plev", "hyam", "finite", "aligned", "overlaps", "range",
         "positive")

# (binding module, symbol, [(argument, kind)] in the order of the header); device and stream are not stored
ENTRY = {
    "temxv": ("_vert", "temxv_interp", [
        ("nf", "int"), ("src", "ptrs"), ("dst", "ptrs"), ("dtype", "int"), ("ncol", "int"), ("nlev", "int"), ("nt", "int"),
        ("nplev", "int"), ("plev", "doubles"), ("pmode", "int"), ("hyam", "doubles"), ("hybm", "doubles"),
        ("p0", "double"), ("ps", "ptr"), ("pdt", "int"), ("method", "int"), ("edge", "int")]),
    "temxl": ("_layout", "temxl_to_engine", [
        ("nf", "int"), ("src", "ptrs"), ("sdt", "ints"), ("dst", "ptrs"), ("ddt", "int"), ("ncol", "int"), ("nlev", "int"),
        ("nt_src", "int"), ("t0", "int"), ("ntb", "int"), ("flags", "int")]),
    "temxi": ("_ingest", "temxi_records_to_pressure", [
        ("nf", "int"), ("src", "ptrs"), ("sdt", "ints"), ("dst", "ptrs"), ("ddt", "int"), ("ncol", "int"), ("nlev", "int"),
        ("nt_src", "int"), ("t0", "int"), ("ntb", "int"), ("nplev", "int"), ("plev", "doubles"), ("hyam", "doubles"),
        ("hybm", "doubles"), ("p0", "double"), ("ps", "ptr"), ("pdt", "int"), ("method", "int"), ("edge", "int")]),
    "temxc": ("_clim", "temxc_time_sum", [
        ("nf", "int"), ("src", "ptrs"), ("sdt", "ints"), ("acc", "ptrs"), ("ncol", "int"), ("nlev", "int"), ("nt", "int"),
        ("flags", "int")]),
}
_ARRAY = {"ptrs": C.c_void_p, "ints": C.c_int, "doubles": C.c_double}


def call_case(fn, args, defaults):
    """One call of entry point ``fn`` with ``defaults`` overridden by ``args`` (arrays as lists, a null pointer as
    None) -> (return code, temx_last_error() as str)."""
    import importlib
    module, symbol, params = ENTRY[fn]
    lib = importlib.import_module("pytemdiags_amd." + module).load()
    a = dict(defaults, **args)
    assert set(a) == {n for n, _ in params}, (fn, sorted(a))
    c = []
    for name, kind in params:
        v = a[name]
        if kind in _ARRAY:
            c.append(None if v is None else (_ARRAY[kind] * len(v))(*v))
        elif kind == "ptr":
            c.append(None if v is None else C.c_void_p(v))
        else:
            c.append(float(v) if kind == "double" else int(v))
    rc = getattr(lib, symbol)(99, *c, None)
    return rc, lib.temx_last_error().decode()


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("fn", ["temxl", "temxi", "temxc"])
def test_refusals_equal_those_recorded_before_the_move_to_the_byte(recorded, fn):
    cases = recorded["cases"][fn]
    replayed = 0
    for case in cases:
        rc, msg = call_case(fn, case["args"], recorded["defaults"][fn])
        assert rc == case["rc"], (case, rc, msg)
        if rc != -2:                                   # the text of a HIP error belongs to the runtime
            assert msg == case["msg"], (case, msg)
        replayed += 1
    assert replayed == recorded["count"][fn] == len(cases) and replayed >= 60
    assert sum(1 for c in cases if c["rc"] == -2) >= 10 and sum(1 for c in cases if c["rc"] == -1) >= 40


def test_temxv_refusals_keep_their_codes_indices_and_key_words(recorded):
    """temxv_interp took the wording of the other three: the code is the recorded one, and every integer and every key
    word of the recorded message is in the new one."""
    cases = recorded["cases"]["temxv"]
    replayed = 0
    for case in cases:
        rc, msg = call_case("temxv", case["args"], recorded["defaults"]["temxv"])
        assert rc == case["rc"], (case, rc, msg)
        if rc == -1:
            have = re.findall(r"\d+", msg)
            for number in re.findall(r"\d+", case["msg"]):
                assert number in have, (case, msg)
            for word in WORDS:
                assert word not in case["msg"] or word in msg, (word, case, msg)
        replayed += 1
    assert replayed == recorded["count"]["temxv"] == len(cases) and replayed >= 60
    assert sum(1 for c in cases if c["rc"] == -2) >= 10 and sum(1 for c in cases if c["rc"] == -1) >= 40


def test_temxv_refuses_a_product_of_sizes_above_2_to_48(recorded):
    """ncol = 2^40, nlev = 2^20 and nt = 2^31 are each in range.  Before the rules were shared temxv_interp had no cap on
    their product: the byte counts of its aliasing check wrapped to zero and this call came back -2, from the device."""
    d = recorded["defaults"]["temxv"]
    rc, msg = call_case("temxv", dict(ncol=1 << 40, nlev=1 << 20, nt=1 << 31, nplev=2), d)
    assert rc == -1 and "range" in msg and "2^48" in msg, (rc, msg)
    # the product counts the longer of the two columns, and 2^48 itself is taken
    rc, msg = call_case("temxv", dict(ncol=1 << 40, nlev=2, nt=1 << 9, nplev=1 << 20), d)
    assert rc == -1 and "range" in msg, (rc, msg)
    far = dict(src=[1 << 60], dst=[1 << 56], ps=1 << 62)
    assert call_case("temxv", dict(far, ncol=1 << 40, nlev=2, nt=1 << 7, nplev=2), d)[0] == -2
    assert call_case("temxv", dict(far, ncol=1 << 40, nlev=2, nt=(1 << 7) + 1, nplev=2), d)[0] == -1


@pytest.mark.parametrize("fn,out", [("temxv", "dst"), ("temxl", "dst"), ("temxi", "dst"), ("temxc", "acc")])
def test_an_extent_that_reaches_the_top_of_the_address_space_does_not_wrap(recorded, fn, out):
    """A source whose last element lies at 2^64 - 8 ends at 2^64.  The sum address + bytes wrapped to 0 there, the
    overlap test said no, and the calls refused here came back -2 before the rules were shared."""
    d = recorded["defaults"][fn]
    src_bytes = {"temxv": 192, "temxl": 480, "temxi": 480, "temxc": 480}[fn]
    top = (1 << 64) - src_bytes
    for at in (top + src_bytes - 8, top + 8, top):
        rc, msg = call_case(fn, dict(src=[top], **{out: [at]}), d)
        assert rc == -1 and "%s 0 overlaps src 0" % out in msg, (at, rc, msg)
    # a source that would run 16 bytes past the top is taken as reaching it, not as coming round to address 0
    assert call_case(fn, dict(src=[top + 16], **{out: [8]}), d)[0] == -2
    # one element lower nothing wraps: refused before the move too
    rc, msg = call_case(fn, dict(src=[top - 8], **{out: [top - 16]}), d)
    assert rc == -1 and "overlaps src 0" in msg, (rc, msg)
    out_bytes = {"temxv": 128, "temxl": 192, "temxi": 128, "temxc": 96}[fn]
    assert call_case(fn, dict(src=[top - 8], **{out: [top - 8 - out_bytes]}), d)[0] == -2       # touching from below


def test_no_second_copy_of_the_rules_is_left_in_temx_hip():
    src = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "temx.hip")).read()
    hpp = open(os.path.join(ROOT, "pytemdiags_amd", "csrc", "field_args.hpp")).read()
    for text in ("auto overlap", "finite and strictly ascending", "is not aligned to its element size", "does not narrow",
                 "entry %d is not finite", "push_back((double)method)"):
        assert text not in src, text
    assert hpp.count("finite and strictly ascending") == 1 and hpp.count("push_back((double)method)") == 1 and not re.search(r"#include\s*<hip", hpp)
    assert re.findall(r'#include "([^"]+)"', hpp) == ["../../include/temx_vert.h"]
    assert '#include "field_args.hpp"' in src


# ---- field_args.hpp on its own, under the sanitizers -----------------------------------------------------------------
def test_aliasing_check_equals_a_128_bit_interval_test_and_the_packer_its_layout(tmp_path):
    """tests/host/field_args_main.cpp: the aliasing check for nf = 1..8, both element sizes and every placement of one
    pair of extents (disjoint, touching, overlapping by one element, nested, at both ends of the address space) against
    an interval test in 128-bit arithmetic; the level tables for nlev = 2, 3, 72, nplev = 1, 2, 30 and both methods."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")
    exe = str(tmp_path / "field_args_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                    os.path.join(ROOT, "tests", "host", "field_args_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"alias_cases=(\d+) refused=(\d+) table_cases=(\d+) mixed_cases=(\d+)", out.stdout)
    assert m, out.stdout
    # nf (nf - 1) / 2 pairs of outputs, nf^2 of an output and a source, nf of an output and the extra input, summed
    # over nf = 1..8, for 2 element sizes, 3 bases and 9 placements; and once per nf and element size no pair at all
    pairs = sum(nf * (nf - 1) // 2 + nf * nf + nf for nf in range(1, 9))
    assert int(m.group(1)) == pairs * 2 * 3 * 9 + 8 * 2
    assert 0 < int(m.group(2)) < int(m.group(1))
    assert int(m.group(3)) == 3 * 3 * 2 and int(m.group(4)) == 23
