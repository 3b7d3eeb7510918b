"""CPU tier of the record layout: the words of a path record and of a transcript-stream record are named once (the ALD_REC_* / ALD_TS_*
enums of include/aletsch_decomp.h; accessors and the two translations in aletsch_amd/csrc/record_layout.h).

 - tests/host_adapter/record_layout_test.cc states both headers by hand, word for word, and checks every accessor and both translations
   (path record -> stream header, stream record -> scratch record header) against them; built plain and with ASan + UBSan, run as the
   stand-alone program it is.
 - the constants of aletsch_amd/distributed.py equal the enum values parsed out of the public header.
 - distributed.parse_records on a hand-written pool of one padded and one unpadded record."""
import os
import re
import subprocess

import numpy as np
import pytest

import common

ROOT = common.ROOT


def _build(flags, name):
    out = os.path.join(ROOT, "tests", "_build"); os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                        os.path.join(ROOT, "tests", "host_adapter", "record_layout_test.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_compiled_layout(sanitize):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    exe = _build(flags, "record_layout_test_san" if sanitize else "record_layout_test")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "record layout ok" in r.stdout, r.stdout + r.stderr


def _header_enums():
    txt = open(os.path.join(ROOT, "include", "aletsch_decomp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"\b(ALD_(?:REC|TS)_[A-Z0-9]+)\s*=\s*(\d+)", txt)}


def test_python_constants_equal_the_header():
    import aletsch_amd.distributed as D
    enums = _header_enums()
    # the two formats as the header's prose has them (an f64 takes two words)
    assert [enums["ALD_REC_" + n] for n in ("GRAPH", "PATH", "NV", "LENGTH", "COUNT", "STRAND", "WEIGHT", "ABD", "CONF", "READS", "NEXW", "HDR")] == [0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16]
    assert [enums["ALD_TS_" + n] for n in ("GRAPH", "PATH", "SID", "STRAND", "COUNT1", "NEXONS", "WEIGHT", "CONF", "ABD", "HDR")] == [0, 1, 2, 3, 4, 5, 6, 8, 10, 12]
    assert len(enums) == 22
    for k, v in enums.items():
        assert getattr(D, k) == v, k
    assert sorted(n for n in dir(D) if n.startswith(("ALD_REC_", "ALD_TS_"))) == sorted(enums)
    assert D.REC_HDR_WORDS == enums["ALD_REC_HDR"]


def test_parse_records_on_a_hand_written_pool():
    from aletsch_amd.distributed import parse_records

    def f64(x):
        return np.array([x], np.float64).view(np.uint32).tolist()

    # graph 1, path 0: 3 vertices, 2 exons -> 16 + 3 + 4 = 23 words, padded to 24
    a = [1, 0, 3, 11, 7, ord("-") | (3 << 8)] + f64(1.5) + f64(2.25) + f64(0.625) + f64(9.75) + [4, 0] + [0, 4, 8] + [100, 200, 300, 400] + [0]
    # graph 0, path 2: 2 vertices, 1 exon -> 16 + 2 + 2 = 20 words, no padding
    b = [0, 2, 2, 5, 1, ord("+")] + f64(3.5) + f64(0.125) + f64(0.75) + f64(6.0) + [2, 0] + [0, 9] + [10, 20]
    assert len(a) == 24 and len(b) == 20
    got = parse_records(np.array(a + b, np.uint32))
    assert got == [dict(graph=0, index=2, length=5, count=1, strand="+", attempt=0, weight=3.5, abd=0.125, conf=0.75, reads=6.0, v=[0, 9], exons=[[10, 20]]),
                   dict(graph=1, index=0, length=11, count=7, strand="-", attempt=3, weight=1.5, abd=2.25, conf=0.625, reads=9.75, v=[0, 4, 8], exons=[[100, 200], [300, 400]])]
