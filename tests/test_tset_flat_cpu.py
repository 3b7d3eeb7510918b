"""CPU tier: the flat transcript set's column view, row operations and merge order (aletsch_amd/csrc/tset_flat.h) under ASan + UBSan.

tests/flat_rows_main.cc is a stand-alone program over that header and the host sink only: an empty set, an item without a sample, the
item without an exon (bucket 0) alone and among others, one exon and nine, sink -> rows -> sink_item -> a fresh sink, the wire form, and
the merge order of two and three sources.  It fails on a wrong result (exit status 1) and on any sanitizer report."""
import os
import subprocess

import common


def test_flat_rows_under_the_sanitizers():
    out = os.path.join(common.ROOT, "tests", "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "flat_rows")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(common.ROOT, "tests", "flat_rows_main.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "flat rows ok" in r.stdout, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
