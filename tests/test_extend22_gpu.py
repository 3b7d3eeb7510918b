"""GPU tier of the extend of a 2-in / 2-out unsplittable vertex: the batches of tests/extend22_cases.py through the product library in
classes 0, 1, 2 and in the twin of class 7 (class 11, hot state in the slab), the hubs of (a), (f), (g) through the raw-form kernels of the
same classes, and one slice of the bench shape, against the oracle:
records (conf through the device's log / exp: 1e-9, everything else bit for bit), iteration counts and the op trace of every graph."""
from __future__ import annotations

import pytest

import aletsch_amd as A
import common
import device_run as DR
import extend22_cases as X

pytestmark = pytest.mark.gpu

KERNELS = DR.forced_kernels((0, 1, 2), twins=(11,))[0]     # (first class, ALD_DEBUG_TWIN, the class the graphs must end in)


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_batch_matches_the_oracle_in_every_class(name):
    pg, prm, (want, st, traces), hits = X.batch(name)
    assert hits > 0
    cap = max(len(t) for t in traces) + 8
    for first, twin, cls in KERNELS:
        natural = int(pg.g_nv.max()) > 32 and cls == 0                       # the 63 / 64-vertex batches do not fit class 0: they run in class 1
        r = DR.run(pg, prm, first=first, twin=twin, trace_cap=cap)
        bad = DR.oracle_mismatches(f"{name}, class {cls}", r, want, st[:, 3], traces, want_classes={1 if natural else cls: pg.n})
        assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"


def test_no_room_for_two_vertices_climbs_a_class():
    """63 vertices started in class 0 (ALD_DEBUG_UNDERCLASS): the fixed form declines, the generic form reports the capacity exit, the
    graph is re-queued one class up and ends with the oracle's records"""
    pg, prm, (want, st, traces), _ = X.batch("i_63_vertices")
    r = DR.run(pg, prm, env={"ALD_DEBUG_UNDERCLASS": "1"})
    assert not DR.oracle_mismatches("i_63_vertices, one class too low", r, want, st[:, 3])


@pytest.mark.parametrize("name", X.RAW_CASES)
def test_raw_form_kernels(name):
    """the hubs of (a), (f) and (g) handed over raw, through the raw-form kernels of classes 0, 1, 2 and 11, against the oracle's pre-steps
    + decomposition"""
    items, spg, (want, st, traces) = X.raw_batch(name)
    cap = max(len(t) for t in traces) + 8
    for first, twin, cls in KERNELS:
        r = DR.run(items, X.params_of(name), first=first, twin=twin, raw=True, trace_cap=cap)
        bad = DR.oracle_mismatches(f"{name}, raw class {cls}", r, want, st[:, 3], traces, want_classes={cls: len(items)})
        assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"


def test_a_slice_of_the_bench_shape():
    pg = A.synth(seed=1002, n_graphs=2000, v_min=64, v_max=64, fixed_edges=256)
    want, st, _, traces = common.oracle_run(pg, threads=8, trace=True)
    assert sum(1 for t in traces for op in t if op[0] in (X.OP_NOW, X.OP_BEST)) >= 10000
    r = DR.run(pg, trace_cap=max(len(t) for t in traces) + 8)
    bad = DR.oracle_mismatches("bench slice", r, want, st[:, 3], traces)
    assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"
