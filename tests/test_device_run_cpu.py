"""The comparator of the GPU parity tests (tests/device_run.py) against itself: DeviceRun records built by hand from the oracle's answer on eight
small graphs -- the identical record has no mismatch, and every single perturbation is reported, under its own label and under no other."""
import dataclasses

import numpy as np
import pytest

import aletsch_amd as A
import common
import device_run as DR

_CACHE = {}


def oracle():
    if not _CACHE:
        pg = A.synth(seed=1001, n_graphs=8, v_min=12, v_max=12, fixed_edges=30)
        want, st, _, traces = common.oracle_run(pg, trace=True)
        assert (want.status == 0).all() and (np.diff(want.path_offset) > 0).all() and min(len(t) for t in traces) >= 2
        _CACHE.update(want=want, iters=st[:, 3].copy(), traces=traces)
    return _CACHE["want"], _CACHE["iters"], _CACHE["traces"]


def identical():
    want, iters, traces = oracle()
    return DR.DeviceRun(dataclasses.replace(want), iters.copy(), {0: 8}, {0: 1}, [list(t) for t in traces])


def mismatches(run, want=None, **kw):
    w, iters, traces = oracle()
    return DR.oracle_mismatches("tag", run, w if want is None else want, iters, traces, want_classes={0: 8}, **kw)


def changed(a, k, v):
    a = a.copy(); a[k] = v
    return a


def test_first_divergence():
    assert DR.first_divergence([1, 2, 3], [1, 2, 3]) == 3
    assert DR.first_divergence([1, 2, 3], [1, 5, 3]) == 1
    assert DR.first_divergence([1, 2], [1, 2, 3]) == 2 and DR.first_divergence([1, 2, 3], [1, 2]) == 2
    assert DR.first_divergence([], [1]) == 0


def test_the_identical_record_has_no_mismatch():
    assert mismatches(identical()) == []
    assert mismatches(identical(), skip_failed=True) == []
    run = identical(); idx = np.array([5, 2, 7])                      # three graphs of the eight, out of order, their traces looked up through `traced`
    want, iters, traces = oracle()
    sub = run._replace(result=common.select_results(want, np.sort(idx)), iterations=iters[np.sort(idx)], traces=[list(traces[g]) for g in np.sort(idx)])
    assert DR.oracle_mismatches("tag", sub, common.select_results(want, np.sort(idx)), iters[np.sort(idx)], traces, traced=np.sort(idx), want_classes={0, 1}) == []
    assert [b[1] for b in DR.oracle_mismatches("tag", sub, common.select_results(want, np.sort(idx)), iters[np.sort(idx)], traces, traced=idx)] == ["trace of graph 5", "trace of graph 2"]


PERTURBATIONS = ("status", "weight", "iterations", "trace op", "truncated trace", "class count", "class outside the set", "failed graph publishes")


@pytest.mark.parametrize("what", PERTURBATIONS)
def test_a_single_perturbation_is_reported_under_its_own_label(what):
    want, iters, traces = oracle(); run = identical(); res = run.result; kw = {}; w = None
    if what == "status":
        run = run._replace(result=dataclasses.replace(res, status=changed(res.status, 3, 1))); expect = ("tag", "status of graph 3", 0, 1)
    elif what == "weight":
        i = int(res.path_offset[4]); x = float(res.weight[i])
        run = run._replace(result=dataclasses.replace(res, weight=changed(res.weight, i, x * (1.0 + 1e-6)))); expect = ("tag", "records", 4, "weight", x, x * (1.0 + 1e-6))
    elif what == "iterations":
        run = run._replace(iterations=changed(iters, 2, iters[2] + 1)); expect = ("tag", "iterations", [2])
    elif what == "trace op":
        c, a, b, v = traces[6][1]; run.traces[6][1] = (c, a + 1, b, v)
        expect = ("tag", "trace of graph 6", "first divergence at 1", (c, a + 1, b, v), traces[6][1])
    elif what == "truncated trace":
        del run.traces[1][-1]; n = len(traces[1]) - 1
        expect = ("tag", "trace of graph 1", "first divergence at %d" % n, None, traces[1][n])
    elif what == "class count":
        run = run._replace(classes={0: 7, 1: 1}); expect = ("tag", "classes", {0: 7, 1: 1}, {0: 8})
    elif what == "class outside the set":
        run = run._replace(classes={0: 7, 2: 1}); kw = dict(want_classes={0, 1}); expect = ("tag", "classes", {0: 7, 2: 1}, [0, 1])
    else:                                                             # no graph of the batch fails: graph 5 is marked failed on both sides, and its paths are still there
        w = dataclasses.replace(want, status=changed(want.status, 5, 100)); run = run._replace(result=dataclasses.replace(res, status=w.status.copy()))
        expect = ("tag", "a failed graph published a path", 5)
    got = DR.oracle_mismatches("tag", run, want if w is None else w, iters, traces, **dict(dict(want_classes={0: 8}), **kw))
    assert got == [expect], got


def test_skip_failed_leaves_out_the_failed_graphs_only():
    """iterations and traces of a graph whose wanted status is >= 100 are not compared under skip_failed; those of every other graph are"""
    want, iters, traces = oracle()
    rest = common.select_results(want, np.array([g for g in range(8) if g != 5]))
    # graph 5 as a failed graph without paths, on both sides
    res = dataclasses.replace(rest, status=changed(want.status, 5, 100), path_offset=np.insert(rest.path_offset, 5, rest.path_offset[5]))
    run = identical()._replace(result=res, iterations=changed(iters, 5, iters[5] + 3))
    run.traces[5] = run.traces[5][:1]
    assert DR.oracle_mismatches("tag", run, res, iters, traces, skip_failed=True) == []
    assert [b[1] for b in DR.oracle_mismatches("tag", run, res, iters, traces)] == ["iterations", "trace of graph 5"]
    run.traces[6] = run.traces[6][:1]
    assert [b[1] for b in DR.oracle_mismatches("tag", run, res, iters, traces, skip_failed=True)] == ["trace of graph 6"]
