"""The launchers' dispatch (pytemdiags_amd/csrc/dispatch.hpp): the lists of values the kernels are instantiated for, each
written once, and the functions that turn a runtime value into a template argument -- on their own under
AddressSanitizer + UBSan (tests/host/dispatch_main.cpp), and the launchers of temx.hip built on them.  Needs no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytemdiags_amd", "csrc")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def test_every_value_reaches_its_constant_and_every_other_value_the_last(tmp_path):
    """tests/host/dispatch_main.cpp: every list entry, values below, between and above each list, the strict pairs of
    the single sweep over a 19 x 19 square, and seven dtypes."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("AddressSanitizer does not start behind another preloaded library")
    exe = str(tmp_path / "dispatch_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *SANITIZE,
                    os.path.join(ROOT, "tests", "host", "dispatch_main.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.search(r"lists=(\d+) probes=(\d+) pairs=(\d+) dtypes=(\d+)", out.stdout)
    assert m, out.stdout
    # seven values outside or around each list, its entries, and one value inside every gap between two entries
    entries, gaps = 4 + 4 + 3 + 3 + 4 + 3, 3 + 2 + 1 + 2 + 3 + 0
    assert [int(g) for g in m.groups()] == [6, 6 * 7 + entries + gaps, 19 * 19, 7]


def test_the_lists_are_written_once_and_no_launch_macro_is_left():
    src = open(os.path.join(CSRC, "temx.hip")).read()
    hpp = open(os.path.join(CSRC, "dispatch.hpp")).read()
    assert not re.search(r"#\s*define\s+TEMX_(L|BIN_|BASIS)", src)
    assert '#include "dispatch.hpp"' in src and not re.search(r"#include\s*<hip", hpp)
    assert re.findall(r'#include "([^"]+)"', hpp) == ["../../include/temx.h"]
    for values in ("4, 8, 13, 16", "2, 4, 7, 8", "1, 2, 4", "8, 10, 12", "16, 32, 48, 64", "2, 3, 4"):
        assert hpp.count("IntList<%s>" % values) == 1, values
    assert src.count('"dtype must be TEMX_F64 or TEMX_F32"') == 1
