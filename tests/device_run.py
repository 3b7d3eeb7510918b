"""One device run and one comparison with the oracle for every GPU parity test (and for the child-process tools under tools/ that run
the same batches through a variant library): how a size class is forced, how a batch goes through DecompBatch, what is read back, and
what `equal to the oracle` means.  A family keeps its graphs, its cached oracle answers and its census; it calls run() and
oracle_mismatches() and adds nothing of its own to either.  Importing this module touches no GPU."""
from __future__ import annotations

import contextlib
import os
from typing import NamedTuple

import numpy as np

import aletsch_amd as A
import common

THREADS = max(1, min(16, len(os.sched_getaffinity(0))))     # host threads of an oracle run
N_CLASSES = 14
HUGE_BATCH = 32                             # class 13: ~105 MB of slab per wave, so no batch of it holds more than 32 graphs
TWIN_OF = {11: 7, 12: 8}                    # a slab twin is reached as its LDS class with ALD_DEBUG_TWIN=1


def forced_kernels(classes, twins=()):
    """-> (rows of (ALD_DEBUG_FIRST_CLASS, ALD_DEBUG_TWIN, the class the graphs must end in), pytest ids): the plain classes, then the twins asked for"""
    rows = [(c, "0", c) for c in classes] + [(TWIN_OF[t], "1", t) for t in twins]
    return rows, ["class%d" % r[2] for r in rows]


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}                 # what the caller had set is put back, not dropped
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def forced_class(first, twin="0", **extra_env):
    """context: ALD_DEBUG_FIRST_CLASS (decomp_common.h: debug_first_class gives pick_class() its first class) and ALD_DEBUG_TWIN set, plus any
    further debug variable (ALD_WG_PER_CU, ALD_DEBUG_UNDERCLASS); on the way out every one of them is what it was before"""
    return _environ(dict(extra_env, ALD_DEBUG_FIRST_CLASS=str(first), ALD_DEBUG_TWIN=twin))


class DeviceRun(NamedTuple):
    result: object                          # DecompResult
    iterations: np.ndarray
    classes: dict                           # class -> graphs that ran in it (classes without a graph left out)
    waves: dict                             # class -> blocks of its last launch (the same classes)
    traces: list                            # per graph [(code, a, b, value)]; empty when nothing was traced


def run(pg_or_items, params=None, *, first=None, twin="0", raw=False, trace_cap=0, env=None) -> DeviceRun:
    """one fresh DecompBatch through the library the process has loaded.  first: the forced first class (None: the environment stays as the
    caller has it); raw: a PackedGraphs goes through add_packed_raw, a list of (pg, phases, dist) through add_raw; trace_cap: events kept
    per graph (0: no trace, as the product runs); env: further variables for this run alone"""
    ctx = forced_class(first, twin, **(env or {})) if first is not None else _environ(dict(env or {}))
    with ctx, A.DecompBatch(0, params, trace_events=trace_cap) as b:
        if not raw: b.add(pg_or_items)
        elif isinstance(pg_or_items, (list, tuple)):
            for pg, phases, dist in pg_or_items:
                assert b.add_raw(pg, phases, dist) == 0
        else: b.add_packed_raw(pg_or_items, 10000)
        b.upload(); b.run(); b.download()
        info = {c: b.class_info(c) for c in range(N_CLASSES)}; info = {c: i for c, i in info.items() if i["n_graphs"]}
        traces = [[(c, x, y, v) for c, x, y, v in b.trace(g)] for g in range(b.n)] if trace_cap else []
        return DeviceRun(b.result(), b.iterations(), {c: i["n_graphs"] for c, i in info.items()}, {c: i["blocks_last_run"] for c, i in info.items()}, traces)


def first_divergence(a, b) -> int:
    """the first index at which two op traces differ; the shorter length when one is a prefix of the other"""
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def in_chunks(n, cls):
    """index arrays that cover range(n): one, or for class 13 pieces of HUGE_BATCH graphs at most"""
    step = HUGE_BATCH if cls == 13 else max(n, 1)
    return [np.arange(a, min(a + step, n)) for a in range(0, n, step)]


def oracle_mismatches(tag, run, want, want_iters=None, want_traces=None, *, want_classes=None, traced=None, skip_failed=False) -> list:
    """THE comparison of a device run with the oracle -> list of differences, each a tuple (tag, label, ...), in this order:
      "status of graph g"                  the status words are equal
      "records"                            common.compare_results, conf within 1e-9 relative (libm against the device's exp / log), all else bit for bit
      "a failed graph published a path"    no path from a graph whose wanted status is >= 100
      "iterations"                         main-loop rule firings per graph (want_iters None: not compared)
      "trace of graph g"                   the WHOLE op trace -- it must end where the oracle's ends -- with the index of the first divergence and
                                           the two ops there (want_traces None: not compared)
      "classes"                            want_classes a dict: {class: graphs} exactly; a set: no graph ran outside it (None: not compared)
    want, want_iters hold the graphs of the run in its order.  traced: the run's graph k is graph traced[k] of want_traces (None: graph k).
    skip_failed: iteration counts and traces of the graphs whose wanted status is >= 100 are left out."""
    got = run.result; n = len(want.status); bad = []
    if np.array_equal(got.status, want.status):
        bad += [(tag, "records") + tuple(x) for x in common.compare_results(want, got, n, conf_tol=1e-9)]
    else:
        g = int(np.nonzero(got.status != want.status)[0][0]); bad.append((tag, "status of graph %d" % g, int(want.status[g]), int(got.status[g])))
    failed = want.status >= 100
    if (np.diff(got.path_offset)[failed] != 0).any():
        bad.append((tag, "a failed graph published a path", int(np.nonzero((np.diff(got.path_offset) != 0) & failed)[0][0])))
    keep = ~failed if skip_failed else np.ones(n, bool)
    if want_iters is not None and not np.array_equal(run.iterations[:n][keep], np.asarray(want_iters)[keep]):
        bad.append((tag, "iterations", np.nonzero((run.iterations[:n] != want_iters) & keep)[0][:5].tolist()))
    if want_traces is not None:
        assert len(run.traces) == n, "the run was not traced"
        for k in np.nonzero(keep)[0]:
            g = int(k if traced is None else traced[k]); mine, ref = run.traces[k], want_traces[g]
            if mine != ref:
                at = first_divergence(mine, ref)
                bad.append((tag, "trace of graph %d" % g, "first divergence at %d" % at, mine[at] if at < len(mine) else None, ref[at] if at < len(ref) else None))
    if isinstance(want_classes, dict):
        if run.classes != {c: k for c, k in want_classes.items() if k}: bad.append((tag, "classes", run.classes, want_classes))
    elif want_classes is not None and not set(run.classes) <= set(want_classes): bad.append((tag, "classes", run.classes, sorted(want_classes)))
    return bad


def class_counts(classes) -> dict:
    """an array of the class each graph must run in -> {class: graphs}, what oracle_mismatches takes as want_classes"""
    return {int(c): int(k) for c, k in zip(*np.unique(classes, return_counts=True))}
