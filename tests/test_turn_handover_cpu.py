"""CPU tier of the hand-over between the trivial-vertex sweep and the smallest-edge sweep (tests/turn_handover_cases.py): the removal of a
smallest edge with the evaluation of its two endpoints alone, and the trivial-vertex scan skipped after the star of a sweep's only candidate.

Neither may change which rule fires when.  Every batch runs through the single-lane emulation -- the plain build and the build that keeps the
sweep records in every class and carries the checkers (a kept record that is stale, or a scan skipped while a type-1 vertex exists, aborts
the process) -- against the oracle, tolerance 0: statuses, records, iteration counts and the op trace (rule, ids and ratio of every firing,
in order).  What a batch is there for is asserted on the oracle's trace and the packed graphs, so that a batch which stops reaching its case
fails instead of passing for nothing.  tests/test_turn_handover_gpu.py runs batches 1 to 4 on the device."""
import ctypes as C

import numpy as np
import pytest

import common
import device_run as DR
import turn_handover_cases as T
from aletsch_amd.packed import export_via


def run_traced(pg, cap, force_class=0, params=None, keep=False):
    """ONE run of the emulation with every graph traced -> (DecompResult, iterations, classes, op traces)"""
    E = common.emu_keep_lib() if keep else common.emu_lib()
    h = C.c_void_p()
    rc = E.emu_run_packed(*pg.c_args(), C.byref(params) if params is not None else None, C.c_int32(cap), C.c_int32(force_class), C.byref(h))
    assert rc == 0, rc
    r = export_via(E.emu_result_export, h, pg.n)
    it = np.zeros(pg.n, np.int32); cl = np.zeros(pg.n, np.int32)
    E.emu_result_iters(h, it.ctypes.data_as(C.POINTER(C.c_int32)), cl.ctypes.data_as(C.POINTER(C.c_int32)))
    traces = [common.emu_trace_of(E, h, g, cap) for g in range(pg.n)]
    E.emu_result_free(h)
    return r, it, cl, traces


def check(name, pg, o, params=None, force_class=0, keep=False, cap=T.TRACE_CAP):
    """statuses, records, iteration counts and the op trace of EVERY graph of the batch against the oracle's"""
    assert max(len(t) for t in o["traces"]) < cap
    got, it, cl, mine = run_traced(pg, cap, force_class, params, keep)
    assert np.array_equal(got.status, o["res"].status), (name, force_class, keep)
    bad = common.compare_results(o["res"], got, pg.n)
    assert not bad, (name, force_class, keep, bad[:3])
    assert np.array_equal(it, o["iters"]), (name, force_class, keep, np.nonzero(it != o["iters"])[0][:10])
    for g in range(pg.n):
        a, b = mine[g], o["traces"][g]
        assert a == b, f"{name}, class >= {force_class}, keep {keep}, graph {g}: first divergence at {DR.first_divergence(a, b)}"
    return cl


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
def test_bench_shape(keep):
    """batch 1: 300 graphs of the benchmark's shape (64 vertices, 256 edges)"""
    pg = T.bench_batch(); o = T.oracle("bench", pg)
    n_small, n_best = T.count(o["traces"], T.OP_SMALLEST) / pg.n, T.count(o["traces"], T.OP_TRIVIAL_BEST) / pg.n
    print(f"\nper graph: {n_small:.1f} SMALLEST, {n_best:.1f} TRIVIAL_BEST, {T.count(o['traces'], T.OP_SMALL_NOW) / pg.n:.1f} SMALL_NOW")
    assert n_small >= 100 and n_best >= 30
    cl = check("bench", pg, o, keep=keep)
    assert (cl == 1).all()


def test_raw_form_of_the_bench_shape():
    """every third graph of batch 1 handed over raw: the pre-steps in the load phase, then the same sweeps, against the oracle's pre-steps +
    decomposition"""
    items, _, staged = T.bench_raw(); o = T.oracle("bench_raw", staged)
    got, it, cl, traces = common.emu_run_raw(items, trace_cap=T.TRACE_CAP, full=True)
    assert not common.compare_results(o["res"], got, len(items))
    assert np.array_equal(it, o["iters"]) and (cl == 1).all()
    assert all(a == b for a, b in zip(traces, o["traces"]))


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
def test_one_chunk_and_the_same_lane_in_two_chunks(keep):
    """batch 2: 32-vertex graphs in class 0; graphs of 100..128 vertices with light edges s -> s + 64 in class 2 (theirs) and in class 3"""
    pg = T.small_batch(); o = T.oracle("small", pg)
    assert T.count(o["traces"], T.OP_SMALLEST) >= 20 * pg.n
    cl = check("small", pg, o, keep=keep)
    assert (cl == 0).all()
    pg, marked = T.far_batch(); o = T.oracle("far", pg)
    hit = sum(1 for g in range(pg.n) if any(ev[0] in (T.OP_SMALL_NOW, T.OP_SMALLEST) and ev[1] in marked[g] for ev in o["traces"][g]))
    print(f"\ngraphs in which an edge s -> s + 64 is removed by the smallest-edge rule: {hit} of {pg.n}")
    assert hit >= 20
    for first in (0, 3):
        cl = check("far", pg, o, force_class=first, keep=keep)
        assert (cl == max(first, 2)).all(), np.unique(cl)


def test_coverage_of_the_hand_made_removals():
    """batch 3, what the oracle did on it: the first firing of every graph is the removal it was built for"""
    hm = T.handmade(); pg = T.pack_dicts([g for _, g in hm]); o = T.oracle("handmade", pg)
    assert (o["res"].status == 0).all()
    f = {name: T.first_removal(g, o["traces"][k]) for k, (name, g) in enumerate(hm)}
    tr = {name: o["traces"][k] for k, (name, _) in enumerate(hm)}
    for name in ("head", "middle", "tail"):
        assert f[name]["out_place"] == f[name]["in_place"] == name and f[name]["out_len"] == f[name]["in_len"] == 3, f[name]
    assert f["leaves_source"]["s"] == 0 and f["enters_sink"]["t"] == f["enters_sink"]["sink"]
    assert f["out_deg_to_1"]["out_len"] == 2 and f["out_deg_to_1"]["in_len"] == 3
    assert f["in_deg_to_1"]["in_len"] == 2 and f["in_deg_to_1"]["out_len"] == 3
    for name in ("out_deg_to_1", "in_deg_to_1"):                # the vertex left with one edge is the trivial vertex of the next firing
        assert tr[name][1][0] in (T.OP_TRIVIAL_NOW, T.OP_TRIVIAL_BEST) and tr[name][1][1] == (f[name]["s"] if name == "out_deg_to_1" else f[name]["t"])
    g = dict(hm)["parallel"]; E = T.sorted_edges(g)
    assert E.count((f["parallel"]["s"], f["parallel"]["t"])) == 2
    # its twin is what both endpoints find next: removed by the very next firing, as the smallest edge of the same vertex
    g = dict(hm)["back_to_the_other_end"]; E = T.sorted_edges(g); a, b = tr["back_to_the_other_end"][:2]
    assert a[0] == b[0] == T.OP_SMALLEST and E[a[1]] == E[b[1]] and a[1] != b[1]
    a, b = tr["two_hits"][:2]
    assert a[0] == b[0] == T.OP_SMALL_NOW and a[2] < b[2]       # two hits of ONE sweep: the second vertex lies behind the first
    # A removal of this rule never takes a degree to 0: its guards ask for out_deg[s] > 1 and in_deg[t] > 1 of the edge it removes.  The
    # degree-0 branch of the removal (maybe_broken) belongs to the cold callers of kill_edge.


def test_coverage_of_the_trivial_cases():
    """batch 4, what the oracle did on it"""
    tc = T.trivial_cases(); tr = {}; gs = {}
    for name, g, prm in tc:
        o = T.oracle("trivial_" + name, T.pack_dicts([g]), prm)
        assert (o["res"].status == 0).all(), name
        tr[name] = o["traces"][0]; gs[name] = g
    triv = (T.OP_TRIVIAL_FAST, T.OP_TRIVIAL_NOW, T.OP_TRIVIAL_BEST)
    deg_in = lambda g, v: sum(1 for a, b in T.sorted_edges(g) if b == v)
    deg_out = lambda g, v: sum(1 for a, b in T.sorted_edges(g) if a == v)

    def one_sided(g):                                            # inner vertices with a single edge on a side, as packed
        return [v for v in range(1, g["V"] - 1) if min(deg_in(g, v), deg_out(g, v)) == 1]
    # The star of the sweep's ONE candidate (vertex 3: vertex 6 is of type 2 until then) makes vertex 6 type 1 through the phasing lists
    # alone -- hs_replace in the star, flags refreshed, another answer to the dominate query --: nothing but the refresh raises maybe_triv
    # again after the early clear (which the DEVICE makes here; see turn_handover_cases.dominate_flip), and the next firing must be vertex 6.  Vertices 1 and 4, whose lists the star edits, keep three edges on
    # that side before and after it (one leaves, one arrives): no degree is at 2 or below even in passing.
    g = gs["dominate_flip"]
    assert one_sided(g) == [3, 6] and deg_out(g, 1) == 3 and deg_out(g, 3) == 2 and deg_in(g, 4) == 3 and deg_in(g, 5) == 4 and deg_out(g, 4) >= 2 and deg_in(g, 6) == 1 and deg_out(g, 6) == 2
    assert [list(v) for v, _ in g["phasing"]] == [[1, 3, 4, 6], [3, 4, 6, 7]]
    assert tr["dominate_flip"][0][:3] == (T.OP_TRIVIAL_BEST, 3, 1) and tr["dominate_flip"][0][3] > tr["dominate_flip"][1][3]     # (6 has the better ratio: it was no candidate of the first scan)
    assert tr["dominate_flip"][1][0] in (T.OP_TRIVIAL_NOW, T.OP_TRIVIAL_BEST) and tr["dominate_flip"][1][1:3] == (6, 1)
    # A dominate query in the SECOND chunk: the scan that completes the sweep starts at vertex 64 and sees one candidate (68) of the two;
    # its count is not one of the whole graph and the flag must stay up -- the best candidate is vertex 4 (its star edits lists of three edges: no degree passes through 1), and 68 is the next firing.
    g = gs["need_in_second_chunk"]
    assert g["V"] > 64 + 2 and one_sided(g) == [4, 68] and deg_out(g, 65) == 3 and deg_out(g, 1) == 3 and deg_in(g, 5) == 3 and [list(v) for v, _ in g["phasing"]] == [[65, 68, 69]]
    assert [ev[:3] for ev in tr["need_in_second_chunk"][:2]] == [(T.OP_TRIVIAL_BEST, 4, 1), (T.OP_TRIVIAL_BEST, 68, 1)]
    # one candidate, chosen at the end of a complete scan, and no trivial vertex after its star: the scan that would find nothing
    assert one_sided(gs["one_candidate"]) == [3]
    assert tr["one_candidate"][0][:3] == (T.OP_TRIVIAL_BEST, 3, 1) and tr["one_candidate"][1][0] not in triv
    # two candidates in the first scan, one in the second
    assert one_sided(gs["two_candidates"]) == [3, 5]
    assert [ev[:3] for ev in tr["two_candidates"][:2]] == [(T.OP_TRIVIAL_BEST, 3, 1), (T.OP_TRIVIAL_BEST, 5, 1)] and tr["two_candidates"][2][0] not in triv
    # the candidate's in-edge 1 -> 3 lies on a phasing path and vertex 1 has another edge out: the scan has to ask (SC_NEED) in the FIRST
    # chunk, is started again at vertex 1 and then counts the whole graph (the clear does happen in phasing_need); the star replaces the two
    # edges of the path by one (hs_replace: flags to refresh)
    for name in ("phasing_need", "phasing_two"):
        g = gs[name]; E = T.sorted_edges(g)
        assert any(list(v[:2]) == [1, 3] for v, _ in g["phasing"]) and sum(1 for a, b in E if a == 1) >= 2 and sum(1 for a, b in E if b == 3) == 1
        assert tr[name][0][:3] == (T.OP_TRIVIAL_BEST, 3, 1)
    assert tr["phasing_two"][1][:3] == (T.OP_TRIVIAL_BEST, 5, 1)
    # a jump ratio above 1: the fast pass (stage 0) fires, and a candidate between 1.02 and the jump ratio ends its scan early
    assert tr["jump_above_one"][0][:3] == (T.OP_TRIVIAL_BEST, 3, 1) and 1.02 <= tr["jump_above_one"][0][3] < 1.5
    assert any(ev[0] == T.OP_TRIVIAL_FAST for ev in tr["jump_above_one"])
    assert all(e[3] != 0 for e in gs["stranded"]["edges"]) and tr["stranded"][0][:3] == (T.OP_TRIVIAL_BEST, 3, 1)


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("first", [0, 2, 10])
def test_hand_made_graphs(first, keep):
    """batches 3 and 4 in classes 0, 2 and 10 (one chunk in registers, several, and the form with the merged list walks)"""
    hm = T.handmade(); pg = T.pack_dicts([g for _, g in hm])
    check("handmade", pg, T.oracle("handmade", pg), force_class=first, keep=keep)
    for name, g, prm in T.trivial_cases():
        pg = T.pack_dicts([g])
        check("trivial_" + name, pg, T.oracle("trivial_" + name, pg, prm), params=prm, force_class=first, keep=keep)


def test_coverage_of_the_fuzz_slice():
    """batch 5, what the oracle did on it: 2 000 graphs of 8..200 vertices in four parts, with and without phasing paths and strands"""
    parts = [T.fuzz_part(k) for k in range(4)]; tr = [t for k, pg in enumerate(parts) for t in T.oracle("fuzz%d" % k, pg)["traces"]]
    nv = np.concatenate([pg.g_nv for pg in parts]); npaths = np.concatenate([pg.g_np for pg in parts])
    assert len(tr) == 2000 and int(nv.min()) <= 12 and int(nv.max()) >= 190
    assert int((npaths > 0).sum()) >= 500 and int((npaths == 0).sum()) >= 500
    assert all((T.oracle("fuzz%d" % k, pg)["res"].status == 0).all() for k, pg in enumerate(parts))
    for code, least in ((T.OP_TRIVIAL_BEST, 10000), (T.OP_TRIVIAL_NOW, 1000), (T.OP_SMALL_NOW, 1000), (T.OP_SMALLEST, 10000)):
        assert T.count(tr, code) >= least, (code, T.count(tr, code))
    # a TRIV_BEST followed at once by another trivial firing, in graphs with phasing paths: the runs the early clear cuts short or must not
    with_paths = [t for k in (1, 3) for t in T.oracle("fuzz%d" % k, parts[k])["traces"]]
    assert sum(1 for t in with_paths for a, b in zip(t, t[1:]) if a[0] == T.OP_TRIVIAL_BEST and b[0] in (T.OP_TRIVIAL_NOW, T.OP_TRIVIAL_BEST)) >= 1000


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("part", range(4))
def test_fuzz_slice(part, keep):
    """batch 5, a quarter at a time: the op trace of every graph"""
    pg = T.fuzz_part(part)
    check("fuzz part %d" % part, pg, T.oracle("fuzz%d" % part, pg), keep=keep, cap=T.FUZZ_TRACE_CAP)
