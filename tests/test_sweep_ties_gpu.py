"""GPU tier of the sweeps' ties, thresholds and lane order: every case of tests/sweep_cases.py against the oracle in each of the 14 plain
kernels, and once more in the natural classes through the WSYNC library.

The three selections of the rule cascade (scan_trivial, the selection loop of sweep_smallest_body, sweep_unsplittable) restate sequential
loops of the reference with ballots, a per-lane fold over the chunks and wave_argmin (a 64-bit minimum made of two 32-bit DPP reductions and
a ballot for the largest tied vertex).  The single-lane emulation runs none of that, so the later-vertex-wins rule, the order of stop and
now lanes, the chunk boundaries and the low word of the minimum are pinned HERE: combs and blocks with ties, exact thresholds and chosen
winner positions, a random batch under the parameters no other test moves, single graphs with a threshold at exactly one of their own ratios.

As in tests/test_class_matrix_gpu.py, ALD_DEBUG_FIRST_CLASS / ALD_DEBUG_TWIN send the graphs to the kernel of one class (a graph larger than
that class runs in its natural class; class 13 in batches of at most 32).  Per graph: the class it ran in, status, records (conf within 1e-9,
as everywhere in this tier), iteration count and the whole op trace -- the trace is the assertion that names the wrong decision.  The raw
builds share the sweeps with the plain ones (the pre-steps run in the load phase, before the first sweep) and are not run here.  The WSYNC
library keeps sweep records in every class and traps if wave_argmin is ever reached with part of the wave switched off."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import class_cases as CC
import common
import device_run as DR
import sweep_cases as SC

pytestmark = pytest.mark.gpu

KERNELS, IDS = DR.forced_kernels(CC.CLASSES, twins=(11, 12))


def test_census_of_the_cases_on_this_machine():
    """the census both tiers assert: counted by the oracle, at least 10 events a line (120 winner positions for line a)"""
    print("\ncensus of the sweep cases (events per line, from the oracle):\n" + SC.census_table())
    assert not SC.census_short(), SC.census_short()
    R = SC.runs(); a, b = R["param/default"], R["param/unread"]       # the indices nothing reads: the oracle's answer is the default's, so the kernel's must be
    assert not common.compare_results(a["res"], b["res"], a["pg"].n) and np.array_equal(a["iters"], b["iters"]) and a["traces"] == b["traces"]


@pytest.mark.parametrize("first,twin,cls", KERNELS, ids=IDS)
def test_plain_kernel_matches_oracle(first, twin, cls):
    t0 = time.perf_counter(); n = 0
    for name, o in SC.runs().items():
        bad = SC.device_mismatches(name, first, cls)
        assert not bad, f"class {cls}: {len(bad)} mismatches, first {bad[:3]}"
        n += o["pg"].n
    print(f"class {cls:2d}: {n} graphs in {len(SC.runs())} runs, 0 mismatches, all traces equal, {time.perf_counter() - t0:.1f} s")


def test_natural_classes_through_the_wsync_build():
    """the WSYNC build: full drain at every hand-over, sweep records kept in every class, and a trap where wave_argmin meets a partial wave"""
    lib = os.path.join(common.ROOT, "aletsch_amd", "lib", "libaletsch_decomp_wsync.so")
    assert os.path.exists(lib), "build it with python __graft_entry__.py"
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "sweep_ties_parity.py"), lib], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-1500:]
    totals = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("TOTAL graphs")]
    assert len(totals) == 1 and totals[0].strip().endswith("mismatches 0"), r.stdout[-2500:]
