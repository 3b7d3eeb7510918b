# the failing graphs of tests/assert_cases.py (every way a star, a router, a sweep and the collect phase end on one of the reference's asserts) GPU vs
# oracle -- status, no path from a failed graph, the whole op trace -- with the first class forced to 0, 1, 2 and the slab twin 11, then the interleaved
# batch (failed graph, witness, ...) in class 2; one library per child process:   python tools/assert_exits_parity.py [lib.so ...]
# (tests/test_assert_exits_gpu.py runs it on the WSYNC=1 and STARREG=1 builds)
import sys
from parity_runner import run_libraries
CHILD = r'''
import assert_cases as AC
tot = 0; nbad = 0
for first, twin, _ in DR.forced_kernels((0, 1, 2), twins=(11,))[0]:
    n, bad = AC.site_mismatches_on_device(first, twin)
    tot += n; nbad += len(bad)
    if bad: print("   mismatch", bad[:3], flush=True)
o = AC.successor_batch()
assert max(len(t) for t in o["traces"]) < AC.TRACE_CAP
r = DR.run(o["pg"], o["params"], first=AC.SUCCESSOR_CLASS, trace_cap=AC.TRACE_CAP)
bad = DR.oracle_mismatches("interleaved", r, o["want"], None, o["traces"])
tot += o["pg"].n; nbad += len(bad)
if bad: print("   mismatch", bad[:3], flush=True)
print("   TOTAL graphs", tot, "mismatches", nbad, flush=True)
sys.exit(0 if nbad == 0 else 1)
'''
sys.exit(run_libraries(CHILD, sys.argv[1:]))
