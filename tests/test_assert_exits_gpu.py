"""GPU tier of the assert exits (tests/assert_cases.py; what the batches reach is asserted in tests/test_assert_exits_cpu.py, on the oracle's site names
and the emulation's lines): the failing graphs through the product library against the oracle -- status word, no path from a failed graph, the
whole op trace of EVERY graph (it must end where the oracle's ends), and the records of the graphs that end well, conf within 1e-9 relative and
everything else bit for bit, as everywhere in this tier.

  * ALD_DEBUG_FIRST_CLASS as in the class matrix: all 14 plain kernels run them (the twins 11 / 12 as 7 / 8 with ALD_DEBUG_TWIN=1); a graph too large
    for a forced class takes its natural class, as it does there.  The classes whose state lives in the wave's slab (10 and 13 with 13 MB and 105 MB a
    wave, and the twins 11 / 12) take an even-stride sample of 80 graphs per parameter set, the site batches only -- what the class matrix runs per
    class; the other classes take every graph;
  * the WSYNC and STARREG builds, one child process each (tools/assert_exits_parity.py);
  * the star and late-exit cases in raw form through the raw build of classes 0 .. 2;
  * the graph behind a failed one.  A wave's successor cannot be chosen here, so it is made likely and checked from the other side: one workgroup
    per CU (ALD_WG_PER_CU=1), the interleaved batch (failed, witness, failed, witness ...) copied until every class that runs has 8 graphs per wave or
    more -- read from the library's diagnostics, not assumed --, run in its order, reversed and in a seeded permutation.  Every graph must give the
    same status, trace and records in all three (conf bit for bit: the device code is the same) and the oracle's.  STATISTICAL: which wave takes
    which graph is the hardware's choice; a witness that depended on its predecessor would show up as a difference between the orders."""
import os
import subprocess
import sys

import numpy as np
import pytest

import assert_cases as AC
import class_cases as CC
import common
import device_run as DR

pytestmark = pytest.mark.gpu

KERNELS, IDS = DR.forced_kernels(CC.CLASSES, twins=(11, 12))


@pytest.mark.parametrize("first,twin,cls", KERNELS, ids=IDS)
def test_failing_graphs_in_every_plain_kernel(first, twin, cls):
    n, bad = AC.site_mismatches_on_device(first, twin, cls)
    assert not bad, bad[:3]
    print(f"class {cls:2d}: {n} graphs that end on an assert, 0 mismatches")


def test_failing_graphs_through_the_variant_builds():
    libs = [os.path.join(common.ROOT, "aletsch_amd", "lib", "libaletsch_decomp_%s.so" % n) for n in ("wsync", "starreg")]
    for lib in libs:
        assert os.path.exists(lib), "build it with python __graft_entry__.py"
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "assert_exits_parity.py"), *libs], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-1500:]
    totals = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("TOTAL graphs")]
    assert len(totals) == 2 and all(ln.strip().endswith("mismatches 0") for ln in totals), r.stdout[-2500:]


def test_star_and_late_exit_cases_in_raw_form():
    """add_packed_raw: the pre-steps run in the load phase of the raw build of classes 0, 1 and 2, then the same exits"""
    raw_pg, staged, labels, dropped = AC.raw_star_and_late_items()
    assert dropped == 0, dropped                                                  # the oracle's pre-steps take every one of them
    assert {int(v) - 3 for v in raw_pg.g_nv} >= set(AC.STAR_FANS)                 # every fan size is there (a star of k has k + 3 vertices)
    want, traces, sites = common.oracle_assert_sites(staged, threads=CC.THREADS)
    assert max(len(t) for t in traces) < AC.TRACE_CAP
    assert (want.status >= 100).sum() >= 0.9 * staged.n and len(set(labels)) >= 8
    for first in (0, 1, 2):
        r = DR.run(raw_pg, first=first, raw=True, trace_cap=AC.TRACE_CAP)
        bad = DR.oracle_mismatches("raw, first class %d" % first, r, want, None, traces, want_classes=set(range(first, DR.N_CLASSES)))
        assert not bad, bad[:3]


def test_three_orders_of_the_interleaved_batch():
    """(see the module text: statistical).  The batch is sized from the grid the diagnostics report."""
    env = {"ALD_WG_PER_CU": "1"}
    o = AC.successor_batch(); pg0 = o["pg"]; prm = o["params"]
    assert max(len(t) for t in o["traces"]) < AC.TRACE_CAP
    sized = DR.run(pg0, prm, first=AC.SUCCESSOR_CLASS, trace_cap=AC.TRACE_CAP, env=env)
    assert set(sized.classes) == {AC.SUCCESSOR_CLASS}, sized.classes             # one class, one work list
    waves = sized.waves[AC.SUCCESSOR_CLASS]                                       # = the CUs of this device once the batch is large enough
    copies = -(-8 * max(waves, 64) // pg0.n) + 1
    o, idx = AC.order_batch(copies)
    rng = np.random.default_rng(6109)
    orders = {"given": np.arange(len(idx)), "reversed": np.arange(len(idx))[::-1], "permuted": rng.permutation(len(idx))}
    runs = {}
    for name, order in orders.items():
        g_of = idx[order]                                                        # position in this run -> graph of the interleaved batch
        r = DR.run(pg0.select(g_of), prm, first=AC.SUCCESSOR_CLASS, trace_cap=AC.TRACE_CAP, env=env)
        n_waves = r.waves[AC.SUCCESSOR_CLASS]
        assert set(r.classes) == {AC.SUCCESSOR_CLASS} and r.classes[AC.SUCCESSOR_CLASS] >= 8 * n_waves, (name, r.classes, r.waves)
        bad = DR.oracle_mismatches(name, r, common.select_results(o["want"], g_of), None, o["traces"], traced=g_of)
        assert not bad, bad[:3]
        back = np.argsort(order, kind="stable")                                   # this run's results in the given order
        runs[name] = (common.select_results(r.result, back), [r.traces[int(k)] for k in back])
    ref, ref_tr = runs["given"]
    for name in ("reversed", "permuted"):
        res, tr = runs[name]
        assert not common.compare_results(ref, res, len(idx)), name              # tolerance 0: conf included
        assert tr == ref_tr, name
    half = int((ref.status != 0).sum())
    assert 0.45 * len(idx) <= half <= 0.55 * len(idx), half                       # half of the graphs fail, half are witnesses
    print(f"\n{len(idx)} graphs x 3 orders in class {AC.SUCCESSOR_CLASS}, {n_waves} waves, {len(idx) / n_waves:.1f} graphs a wave: identical per graph and equal to the oracle")
