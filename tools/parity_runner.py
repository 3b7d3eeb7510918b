# shared by tools/twins_parity.py and tools/hub_parity.py: run one piece of Python (the CHILD, which compares the GPU with the oracle and prints
# a "TOTAL graphs ... mismatches N" line) once per library, each in a child process of its own with ALETSCH_DECOMP_LIB set and a time limit;
# after a child that failed (a mismatch, a GPU fault, the time limit) nothing else is started
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRELUDE = r'''
import sys, os, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import aletsch_amd as A, common, device_run as DR
threads = DR.THREADS
''' % (ROOT, ROOT)


def run_libraries(child, libs, env=None, seconds=240):
    """child: Python source run after PRELUDE; libs: library paths (none: the product library) -> exit code"""
    rc = 0
    for lib in (libs or [os.path.join(ROOT, "aletsch_amd/lib/libaletsch_decomp.so")]):
        print("library", os.path.basename(lib), flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-c", PRELUDE + child],
                           env=dict(os.environ, ALETSCH_DECOMP_LIB=os.path.abspath(lib), **(env or {})), check=False)
        print("   rc", r.returncode, flush=True)
        if r.returncode != 0: rc = 1; break        # (after a GPU fault nothing else is started)
    return rc
