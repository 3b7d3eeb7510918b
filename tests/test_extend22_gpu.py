"""GPU tier of the extend of a 2-in / 2-out unsplittable vertex: the batches of tests/extend22_cases.py through the product library in
classes 0, 1, 2 and in the twin of class 7 (class 11, hot state in the slab), the hubs of (a), (f), (g) through the raw-form kernels of the
same classes, and one slice of the bench shape, against the oracle:
records (conf through the device's log / exp: 1e-9, everything else bit for bit), iteration counts and the op trace of every graph."""
from __future__ import annotations

import numpy as np
import pytest

import aletsch_amd as A
import common
import extend22_cases as X

pytestmark = pytest.mark.gpu

KERNELS = [(0, None, 0), (1, None, 1), (2, None, 2), (7, "1", 11)]     # (first class, ALD_DEBUG_TWIN, the class the graphs must end in)


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_batch_matches_the_oracle_in_every_class(monkeypatch, name):
    pg, prm, (want, st, traces), hits = X.batch(name)
    assert hits > 0
    cap = max(len(t) for t in traces) + 8
    for first, twin, cls in KERNELS:
        monkeypatch.setenv("ALD_DEBUG_FIRST_CLASS", str(first)); monkeypatch.setenv("ALD_DEBUG_TWIN", twin or "0")
        with A.DecompBatch(0, prm, trace_events=cap) as b:
            b.add(pg); b.upload(); b.run(); b.download()
            got = b.result(); it = b.iterations()
            used = {c: b.class_info(c)["n_graphs"] for c in range(14)}
            mine = [[(c, a, bb, v) for c, a, bb, v in b.trace(g)] for g in range(pg.n)]
        natural = int(pg.g_nv.max()) > 32 and cls == 0                       # the 63 / 64-vertex batches do not fit class 0: they run in class 1
        assert used[1 if natural else cls] == pg.n, (name, cls, {c: k for c, k in used.items() if k})
        bad = common.compare_results(want, got, pg.n, conf_tol=1e-9)
        assert not bad, f"{name}, class {cls}: {len(bad)} mismatches, first {bad[:3]}"
        assert np.array_equal(it, st[:, 3]), (name, cls, np.nonzero(it != st[:, 3])[0][:10])
        for g in range(pg.n):
            assert mine[g] == traces[g], f"{name}, class {cls}, graph {g}: first divergence at {next((i for i, (x, y) in enumerate(zip(mine[g], traces[g])) if x != y), min(len(mine[g]), len(traces[g])))}"


def test_no_room_for_two_vertices_climbs_a_class(monkeypatch):
    """63 vertices started in class 0 (ALD_DEBUG_UNDERCLASS): the fixed form declines, the generic form reports the capacity exit, the
    graph is re-queued one class up and ends with the oracle's records"""
    pg, prm, (want, st, traces), _ = X.batch("i_63_vertices")
    monkeypatch.setenv("ALD_DEBUG_UNDERCLASS", "1")
    with A.DecompBatch(0, prm) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        got = b.result(); it = b.iterations()
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)
    assert np.array_equal(it, st[:, 3])


@pytest.mark.parametrize("name", X.RAW_CASES)
def test_raw_form_kernels(monkeypatch, name):
    """the hubs of (a), (f) and (g) handed over raw, through the raw-form kernels of classes 0, 1, 2 and 11, against the oracle's pre-steps
    + decomposition"""
    items, spg, (want, st, traces) = X.raw_batch(name)
    cap = max(len(t) for t in traces) + 8
    for first, twin, cls in KERNELS:
        monkeypatch.setenv("ALD_DEBUG_FIRST_CLASS", str(first)); monkeypatch.setenv("ALD_DEBUG_TWIN", twin or "0")
        with A.DecompBatch(0, X.params_of(name), trace_events=cap) as b:
            for pg, phases, dist in items:
                assert b.add_raw(pg, phases, dist) == 0
            b.upload(); b.run(); b.download()
            got = b.result(); it = b.iterations()
            used = {c: b.class_info(c)["n_graphs"] for c in range(14)}
            mine = [[(c, a, bb, v) for c, a, bb, v in b.trace(g)] for g in range(len(items))]
        assert used[cls] == len(items), (name, cls, {c: k for c, k in used.items() if k})
        bad = common.compare_results(want, got, len(items), conf_tol=1e-9)
        assert not bad, f"{name}, raw class {cls}: {len(bad)} mismatches, first {bad[:3]}"
        assert np.array_equal(it, st[:, 3]), (name, cls)
        for g in range(len(items)):
            assert mine[g] == traces[g], (name, cls, g)


def test_a_slice_of_the_bench_shape():
    pg = A.synth(seed=1002, n_graphs=2000, v_min=64, v_max=64, fixed_edges=256)
    want, st, _, traces = common.oracle_run(pg, threads=8, trace=True)
    assert sum(1 for t in traces for op in t if op[0] in (X.OP_NOW, X.OP_BEST)) >= 10000
    cap = max(len(t) for t in traces) + 8
    with A.DecompBatch(0, trace_events=cap) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        got = b.result(); it = b.iterations()
        mine = [[(c, a, bb, v) for c, a, bb, v in b.trace(g)] for g in range(pg.n)]
    bad = common.compare_results(want, got, pg.n, conf_tol=1e-9)
    assert not bad, f"{len(bad)} mismatches, first {bad[:3]}"
    assert np.array_equal(it, st[:, 3])
    for g in range(pg.n):
        assert mine[g] == traces[g], f"graph {g}: first divergence at {next((i for i, (x, y) in enumerate(zip(mine[g], traces[g])) if x != y), min(len(mine[g]), len(traces[g])))}"
