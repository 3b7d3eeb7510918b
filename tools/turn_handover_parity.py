# the batches of tests/turn_handover_cases.py (smallest-edge removal and the evaluation of its two endpoints; the trivial-vertex scan skipped
# after the star of a sweep's only candidate) GPU vs oracle -- records, iteration counts and the op trace of every graph -- in classes 0, 1, 2
# and the slab twin 11, one library per child process:   python tools/turn_handover_parity.py [lib.so ...]
# (tests/test_turn_handover_gpu.py runs it on the WSYNC=1 and STARREG=1 builds)
import sys
from parity_runner import run_libraries
CHILD = r'''
import turn_handover_cases as T
tot = 0; nbad = 0
for name, pg, prm in T.gpu_batches():
    o = T.oracle(name, pg, prm)
    for first, twin, cls in T.FORCINGS:
        bad = T.mismatches_on_device(name, pg, o, prm, first, twin, cls)
        tot += pg.n; nbad += len(bad)
        if bad: print("   mismatch", bad[:3], flush=True)
print("   TOTAL graphs", tot, "mismatches", nbad, flush=True)
sys.exit(0 if nbad == 0 else 1)
'''
sys.exit(run_libraries(CHILD, sys.argv[1:]))
