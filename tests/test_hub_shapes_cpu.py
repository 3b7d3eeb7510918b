"""CPU tier of the hub shapes (tests/shapes.py): the batch that reaches every star and router form of the kernel.

The kernel picks its code path by the degree of the vertex at hand; which degrees a batch really met is counted in the ORACLE (a census per
run: trivial decompositions by direction and fan size, router builds by in-degree, out-degree, phasing lists, sample sets), never in the
product kernel.  Records that equal the oracle's bit for bit mean the same sequence of graph states, so the oracle's census is the kernel's.
This file asserts that every bucket of that census holds at least MIN_EVENTS events over the hub batch -- with the bucket lines taken from
the kernel headers --, and runs the batch through the single-lane emulation (list build, row build, kept-records build) against the oracle:
records, iteration counts and the op trace.  tests/test_hub_shapes_gpu.py repeats the comparison on the device, where the wave-parallel forms
(star_reg, router_prepare) exist."""
import ctypes as C

import numpy as np
import pytest

import common
import device_run as DR
import shapes

MIN_EVENTS = 10
K = shapes.kernel_constants()


def _oracle(pg, params=None):
    if not hasattr(_oracle, "memo"):
        _oracle.memo = {}
    if id(pg) not in _oracle.memo:
        _oracle.memo[id(pg)] = shapes.census_of(pg, threads=DR.THREADS, params=params)
    return _oracle.memo[id(pg)]


def batches():
    """(name, batch, parameters): the hub batch under the default parameters, the wide routers without phasing lists under theirs"""
    pg, _ = shapes.hub_batch(); wpg, _, wp = shapes.wide_router_batch()
    return (("hubs", pg, None), ("wide routers", wpg, wp))


def emu_traces(pg, rows=False, keep=False, cap=1 << 15, params=None):
    """the emulation's op trace of every graph (rule id, vertex or edge id, second id, ratio of every firing, in order)"""
    E = common.emu_rows_lib() if rows else (common.emu_keep_lib() if keep else common.emu_lib())
    h = C.c_void_p()
    assert E.emu_run_packed(*pg.c_args(), C.byref(params) if params is not None else None, C.c_int32(cap), C.c_int32(0), C.byref(h)) == 0
    out = []
    for g in range(pg.n):
        n = C.c_int32(); E.emu_result_trace(h, g, C.byref(n), None, None, 0)
        assert n.value <= cap, (g, n.value)
        codes = np.zeros(3 * max(1, n.value), np.int32); vals = np.zeros(max(1, n.value))
        E.emu_result_trace(h, g, C.byref(n), codes.ctypes.data_as(C.POINTER(C.c_int32)), vals.ctypes.data_as(C.POINTER(C.c_double)), n.value)
        out.append([(int(codes[3 * i]), int(codes[3 * i + 1]), int(codes[3 * i + 2]), float(vals[i])) for i in range(n.value)])
    E.emu_result_free(h)
    return out


def test_thresholds_come_from_the_kernel_headers():
    """STAR_MAX, LP, the arena sizes, ALD_STARFIX_MAX of every class and the router's `small` test are parsed out of decomp_device.h /
    decomp_common.h (shapes.kernel_constants raises when one is missing); what is checked here is only that they hang together"""
    assert len(K["STARFIX_MAX"]) == K["NUM_CLASSES"] and all(1 <= x <= K["STAR_MAX"] for x in K["STARFIX_MAX"])
    assert len(set(K["STARFIX_MAX"])) == 2                                            # the class groups of the census exist
    assert all(K["STARFIX_MAX"][t] == K["STARFIX_MAX"][c] for c, t in K["TWINS"].items())
    assert K["router_small"](2, 2, False) and K["router_small"](2, 2, True) and not K["router_small"](K["LP"], 2, False)
    assert K["STAR_MAX"] < 64 and K["LP"] <= 64
    # every degree the census has a line at is one the generators build
    assert {K["STAR_MAX"] - 1, K["STAR_MAX"], K["STAR_MAX"] + 1, 63, 64, 65} <= set(shapes.FANS)
    sizes = {a + b for a, b in shapes.ROUTERS}
    assert {K["LP"] - 1, K["LP"], K["LP"] + 1} <= sizes
    assert any(K["router_small"](a, b, False) and not K["router_small"](a + 1, b, False) for a, b in shapes.ROUTERS)
    assert any(K["router_small"](a, b, True) for a, b in shapes.ROUTERS if (a, b) != (2, 2)) and any(not K["router_small"](a, b, True) and a + b <= K["LP"] for a, b in shapes.ROUTERS)


def hub_census():
    cen = None
    for _, pg, prm in batches():
        want, st, per_graph = _oracle(pg, prm)
        _, _, cl = common.emu_run(pg, params=prm)                                      # (the size class of every graph)
        c = shapes.Census(per_graph, cl, pg.g_nv, K)
        cen = c if cen is None else cen.add(c)
    zpg, _ = shapes.zero_count_batch()
    _, _, zper = _oracle(zpg)
    zc = shapes.Census(zper, np.zeros(zpg.n, np.int32), zpg.g_nv, K)
    cen.routers["routes, count 0"] = zc.routers.get("routes, count 0", 0)              # (that bucket is filled by the batch whose graphs may end on an assert)
    import class_cases                                                                 # the group of classes 10 / 13: the small hubs of the class mix, which
    cen.add_group(class_cases.forced_hub_census(K), "10,13")                           # tests/test_class_matrix_*.py run in those classes (pick_class's first class)
    return cen


def test_every_census_bucket_is_filled():
    """Every fan-size bucket in both directions, fans of 2..8 in every class group ALD_STARFIX_MAX distinguishes (graphs of class 0 / 1, of
    classes 2..9, of twin size, and -- from the class mix -- of classes 10 / 13), and every router bucket: at least MIN_EVENTS events each, counted by the oracle over the hub batch."""
    cen = hub_census()
    print("\ncensus of the hub batch (events per bucket):\n" + cen.table())
    short = {k: v for k, v in cen.required().items() if v < MIN_EVENTS}
    assert not short, short


@pytest.mark.parametrize("build", ["lists", "rows", "keep"])
def test_emulation_matches_oracle_on_the_hub_batch(build):
    """records bit for bit, every status 0, iteration counts and the op trace of every graph: list build, adjacency-row build (with its row
    checker), kept-records build (with its stale-record checker)"""
    kw = dict(rows=(build == "rows"), keep=(build == "keep"))
    for name, pg, prm in batches():
        want, st, _ = _oracle(pg, prm)
        got, it, cl = common.emu_run(pg, params=prm, **kw)
        bad = common.compare_results(want, got, pg.n)
        assert not bad, (name, bad[:3])
        assert (want.status == 0).all(), (name, np.nonzero(want.status)[0][:10])
        assert np.array_equal(it, st[:, 3]), name
        traces = common.oracle_run(pg, threads=DR.THREADS, trace=True, params=prm)[3]
        mine = emu_traces(pg, params=prm, **kw)
        for g in range(pg.n):
            assert mine[g] == traces[g], f"{name}, graph {g}: first divergence at {DR.first_divergence(mine[g], traces[g])}"


def test_hub_batch_started_one_class_too_low(monkeypatch):
    """ALD_DEBUG_UNDERCLASS=1: a fan of 300 makes hundreds of edges, so hubs are what outgrows a class; the retry one class up must end with
    the oracle's records"""
    for name, pg, prm in batches():
        want, _, _ = _oracle(pg, prm)
        _, _, cl_plain = common.emu_run(pg, params=prm)
        monkeypatch.setenv("ALD_DEBUG_UNDERCLASS", "1")
        got, _, cl = common.emu_run(pg, params=prm)
        monkeypatch.delenv("ALD_DEBUG_UNDERCLASS")
        assert not common.compare_results(want, got, pg.n), name
        low = np.maximum(cl_plain - 1, 0)
        assert (cl >= low).all() and int((cl > low).sum()) >= 10, (name, int((cl > low).sum()))          # hubs did have to climb


def test_hubs_with_a_zero_count_edge_end_as_the_oracle_does():
    """edge_info.count == 0 on a hub edge (the iso == 2 branch of router_prepare).  Every such graph ends on one of the reference's asserts
    (a merge meets the edge sooner or later), so the records are empty and say nothing about the router: what is compared is the status word
    and the OP TRACE up to the assert -- the router that fired on the hub before it, with its vertex, type and leftover ratio."""
    pg, _ = shapes.zero_count_batch()
    want, st, per_graph = _oracle(pg)
    assert (want.status >= 100).all()
    traces = common.oracle_run(pg, threads=DR.THREADS, trace=True)[3]
    fired = sum(1 for t in traces if any(ev[0] in (7, 8) for ev in t))                # OP_UNSPLIT_NOW / OP_UNSPLIT_BEST
    assert fired >= MIN_EVENTS, fired
    for kw in (dict(), dict(rows=True), dict(keep=True)):
        got, it, _ = common.emu_run(pg, **kw)
        assert not common.compare_results(want, got, pg.n), kw
        mine = emu_traces(pg, **kw)
        for g in range(pg.n):
            assert mine[g] == traces[g], (kw, g)


def test_census_notices_a_missing_generator():
    """the batch without its hubs of STAR_MAX + 1 edges leaves that bucket short: the census condition is not met by the other graphs' leftovers"""
    S = K["STAR_MAX"] + 1
    pg, _ = shapes.hub_batch(without=(S,))
    _, _, per_graph = shapes.census_of(pg, threads=DR.THREADS)
    _, _, cl = common.emu_run(pg)
    req = shapes.Census(per_graph, cl, pg.g_nv, K).required()
    assert min(req["fan %d in" % S], req["fan %d out" % S]) < MIN_EVENTS, (req["fan %d in" % S], req["fan %d out" % S])


def test_raw_hub_graphs_through_the_pre_steps():
    """hub graphs handed over raw (phases as exon-coordinate lists): the load phase folds the boundary edges at the source and the sink,
    which is where hubs live; against the oracle's pre-steps + decomposition"""
    from aletsch_amd.packed import PackedGraphs
    O = common.oracle_lib()
    O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]; O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
    items, staged, ok = raw_items(O)
    got, _ = common.emu_run_raw(items)
    ok = np.array(ok)
    assert ok.sum() >= 0.9 * len(ok)
    want = common.oracle_run(PackedGraphs.concat(staged), threads=DR.THREADS)[0]
    assert not common.compare_results(want, common.select_results(got, np.nonzero(ok)[0]), len(staged), conf_tol=1e-9)
    assert (got.status[~ok] >= 100).all()


def raw_items(O, stride=7):
    """every stride-th graph of the hub batch in raw form -> (items for add_raw / emu_run_raw, the oracle's staged graphs, pre-steps passed?)"""
    import aletsch_amd as A
    _, graphs = shapes.hub_batch()
    items, staged, ok = [], [], []
    for g in graphs[::stride]:
        ends = [(e[0], e[1]) for e in g["edges"] if e[0] == 0 or e[1] == g["V"] - 1]
        if g["V"] > 330 or len(set(ends)) != len(ends):          # (the raw entry point refuses parallel edges at the source / sink: the reference's grouping is undefined on them)
            continue
        pg, phases = shapes.raw_form(g)
        want, _, _, rc = A.pre_assemble(pg, phases, 10000, _lib=O, _prefix="ora")
        items.append((pg, phases, 10000)); ok.append(rc == 0)
        if rc == 0:
            staged.append(want)
    return items, staged, ok
