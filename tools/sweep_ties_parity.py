# the cases of tests/sweep_cases.py (ties, exact thresholds and chosen lane positions in the three selections of the rule cascade) GPU vs oracle
# -- classes, statuses, records, iteration counts and the op trace of every graph -- in the natural classes, one library per child process:
#   python tools/sweep_ties_parity.py [lib.so ...]          (tests/test_sweep_ties_gpu.py runs it on the WSYNC=1 build)
import sys
from parity_runner import run_libraries
CHILD = r'''
import sweep_cases as SC
tot = 0; nbad = 0
for name, o in SC.runs().items():
    bad = SC.device_mismatches(name)
    tot += o["pg"].n; nbad += len(bad)
    if bad: print("   mismatch", bad[:3], flush=True)
print("   TOTAL graphs", tot, "mismatches", nbad, flush=True)
sys.exit(0 if nbad == 0 else 1)
'''
sys.exit(run_libraries(CHILD, sys.argv[1:]))
