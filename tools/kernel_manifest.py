#!/usr/bin/env python3
"""The kernels of a libtemx.so as sorted text, so that two builds can be diffed:

    python tools/kernel_manifest.py pytemdiags_amd/libtemx.so > new.txt ; diff old.txt new.txt

One line per symbol-table entry of a kernel (its code, and its descriptor NAME.kd) with the size, then one line per
kernel with the resources in the code object's metadata note.  A refactor of the host side must leave it unchanged.
Needs llvm-objcopy, clang-offload-bundler and llvm-readelf of ROCm (ROCM_PATH, default /opt/rocm); no GPU."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size",
          ".uses_dynamic_stack")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool), *args], check=True, capture_output=True, text=True).stdout


def manifest(lib):
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib)
        run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co)
        symbols, notes = run("llvm-readelf", "-sW", co), run("llvm-readelf", "--notes", co)
    kernels = {}
    for block in re.split(r"\n  - ", notes.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0]):
        name = re.search(r"\n    \.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = " ".join("%s=%s" % (f[1:], (re.search(re.escape(f) + r":\s+(\S+)", block) or [0, "-"])[1])
                                              for f in FIELDS)
    lines = []
    for row in symbols.splitlines():          # Num: Value Size Type Bind Vis Ndx Name
        col = row.split()
        if len(col) == 8 and col[3] in ("FUNC", "OBJECT") and (col[7] in kernels or col[7][:-3] in kernels and col[7].endswith(".kd")):
            lines.append("symbol %s size=%s %s" % (col[7], col[2], col[3]))
    return sorted(lines) + ["kernel %s %s" % kv for kv in sorted(kernels.items())]


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = manifest(sys.argv[1])
    print("\n".join(out))
    print("# %d symbol entries (%d descriptors), %d kernels" % (sum(x.startswith("symbol") for x in out),
                                                                sum(" size=64 OBJECT" in x for x in out), len(out) - sum(x.startswith("symbol") for x in out)), file=sys.stderr)
