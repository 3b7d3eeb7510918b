"""GPU tier of the hand-over between the trivial-vertex sweep and the smallest-edge sweep: batches 1 to 4 of tests/turn_handover_cases.py
(what they exercise is asserted in tests/test_turn_handover_cpu.py, on the oracle's trace) through the product library against the oracle --
statuses, records, iteration counts and the op trace of EVERY graph -- with the first class forced to 0, 1, 2 and to the slab twin 11, so that
the one-chunk, two-chunk and many-chunk register forms and the slab form of the sweeps all run them; the raw form of batch 1; then the same
batches through the WSYNC and STARREG builds, one child process each.  Records are compared as everywhere in this tier: conf within 1e-9
relative (libm against the device's exp / log), everything else bit for bit."""
import os
import subprocess
import sys

import pytest

import common
import turn_handover_cases as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("first,twin,cls", T.FORCINGS, ids=["class0", "class1", "class2", "twin11"])
def test_batches_match_oracle(first, twin, cls):
    """(the `dominate_flip` case of batch 4 is live HERE: with 64 lanes the dominate queries of its first scan are answered within the first
    chunk, the scan starts again at vertex 1, counts one candidate and the flag is cleared before the star -- only the refreshed phasing
    flags bring it back for the vertex that star turns into a type-1 one)"""
    for name, pg, prm in T.gpu_batches():
        bad = T.mismatches_on_device(name, pg, T.oracle(name, pg, prm), prm, first, twin, cls)
        assert not bad, bad[:3]


def test_raw_form_of_the_bench_batch():
    """add_packed_raw: the pre-steps run in the load phase of the raw build of the kernel, then the same sweeps"""
    items, raw_pg, staged = T.bench_raw()
    o = T.oracle("bench_raw", staged)
    for first, twin, cls in T.FORCINGS[:3]:
        bad = T.mismatches_on_device("bench", raw_pg, o, None, first, twin, cls, raw=True)
        assert not bad, bad[:3]


def test_batches_through_the_variant_builds():
    """the WSYNC build (full drain at every hand-over, kept sweep records in every class) and the STARREG build (fans of 2..4 in registers)"""
    libs = [os.path.join(common.ROOT, "aletsch_amd", "lib", "libaletsch_decomp_%s.so" % n) for n in ("wsync", "starreg")]
    for lib in libs:
        assert os.path.exists(lib), "build it with python __graft_entry__.py"
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "turn_handover_parity.py"), *libs], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-1500:]
    totals = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("TOTAL graphs")]
    assert len(totals) == 2 and all(ln.strip().endswith("mismatches 0") for ln in totals), r.stdout[-2500:]
