"""One seeded mix of SMALL graphs for the size-class matrix (tests/test_class_matrix_cpu.py, tests/test_class_matrix_gpu.py).

The decomposition engine is compiled once per size class, plain and raw, and the source differs by class (width of the creation ids, kept
sweep records, the merged list walks of the slab-resident classes, ALD_STARFIX_MAX, the register form of the sweeps).  pick_class() takes a
FIRST class, so a graph of 6..60 vertices can be run in every one of those kernels; the mix below is what both tiers run there.  It has
three parts:

  staged        A.synth graphs in all three weight modes with 4 samples, 12 phasing paths, strands and touching exons, explicit edge counts
                that differ from the sample counts, permuted creation ranks on a third of them; small hubs of tests/shapes.py (fans of
                1, 2, 3, 4, 5, 8, 16 in both directions: ALD_STARFIX_MAX splits the classes at 2..4; routers 2x2 .. 6x6)
  second set    its own sub-batch under second_params() (ratio[7] = 1.5, ratio[0] = 0.2, max_num_exons = 30): OP_TRIVIAL_FAST and the
                greedy-only path fire; hand-made graphs with a dead-end vertex give OP_BROKEN
  raw           common.gene_like_raw items with distances from 10000 / 150 / 0 and duplicate phases, and small hubs in shapes.raw_form

census() counts what the mix exercised, FROM THE ORACLE ALONE (its op trace, shapes.census_of, its pre-steps): records that equal the
oracle's bit for bit mean the same sequence of graph states, so the oracle's census is the kernel's in every class."""
from __future__ import annotations

import ctypes as C

import numpy as np

import aletsch_amd as A
from aletsch_amd.packed import PackedGraphs
import common
from device_run import THREADS
import shapes

CLASSES = tuple(range(11)) + (13,)          # what pick_class chooses from (the twins 11 / 12 are a placement choice of the GPU host)
MIN_EVENTS = 10
TRACE_STRIDE = 4                            # the op trace is compared on every fourth graph
TRACE_CAP = 1 << 13
FANS = (1, 2, 3, 4, 5, 8, 16)
ROUTERS = ((2, 2), (2, 3), (3, 3), (4, 4), (6, 6))
_CACHE = {}


def second_params():
    """the second parameter set: the fast trivial pass takes vertices up to a balance ratio of 1.5, the smallest-edge rule stops at 0.2,
    and a graph of more than 30 vertices skips the rule cascade (greedy phase only)"""
    p = A.default_params()
    p.max_decompose_error_ratio[7] = 1.5; p.max_decompose_error_ratio[0] = 0.2; p.max_num_exons = 30
    return p


def _synth_part(seed: int, n_each: int, rng, v_max: int = 60):
    """A.synth in the three weight modes, every feature on; explicit edge counts; permuted creation ranks on every third graph"""
    parts = []
    for mode in range(3):
        pg = A.synth(seed=seed + mode, n_graphs=n_each, v_min=6, v_max=v_max, edges_per_vertex=3, phasing_per_graph=12, weight_mode=mode,
                     n_samples=4, strand_mode=1, layout_mode=1)
        pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
        rank = pg.identity_rank().astype(np.int32); sl = pg.graph_slices()
        for g in range(mode % 3, pg.n, 3):
            e0, E = int(sl["e"][g]), int(pg.g_ne[g])
            rank[e0:e0 + E] = rng.permutation(E)
        pg.edge_rank = rank
        parts.append(pg)
    return parts


def _hub_part(seed: int, repeat: int, rng):
    graphs = shapes.star_graphs(seed, fans=FANS, repeat=repeat) + shapes.star_graphs_with_tails(seed + 1, fans=FANS[1:5], repeat=max(1, repeat // 2)) \
        + shapes.router_graphs(seed + 2, routers=ROUTERS, repeat=repeat)
    graphs = [g for g in graphs if g["V"] <= 60]
    return shapes.pack(graphs, rng, set(range(0, len(graphs), 3))), graphs


def staged_batch() -> PackedGraphs:
    """the staged part, run under the default parameters"""
    if "staged" not in _CACHE:
        rng = np.random.default_rng(4101)
        hubs, graphs = _hub_part(4120, 2, rng)
        _CACHE["staged"] = PackedGraphs.concat(_synth_part(4110, 8, rng) + [hubs])
        _CACHE["hub_graphs"] = graphs
    return _CACHE["staged"]


def dead_end_graphs(rng, n: int = 14):
    """hand-made: a chain source -> ... -> sink with side branches, one of which ends in a vertex that has no out-edge (the reference
    removes such a vertex's edges: OP_BROKEN) -- and, on every other graph, one that has no in-edge"""
    out = []
    for r in range(n):
        k = int(rng.integers(4, 9)); V = k + 4                        # chain 1..k, dead end k+1, orphan k+2, sink k+3
        w = float(rng.integers(8, 30)); edges = [[0, 1, w, 0, {0: w}]]
        for i in range(1, k):
            edges.append([i, i + 1, w, 0, {0: w, 1 + r % 3: 2.0}])
        edges.append([k, V - 1, w, 0, {0: w}])
        a = int(rng.integers(1, k)); d = float(rng.integers(1, 6))
        edges.append([a, k + 1, d, 0, {0: d}])                        # into the dead end
        if r % 2:
            edges.append([k + 2, V - 1, d, 0, {0: d}])                # out of a vertex nothing leads to
        else:
            edges.append([0, k + 2, d, 0, {0: d}]); edges.append([k + 2, V - 1, d, 0, {0: d}])
        b = int(rng.integers(1, k - 1)); x = float(rng.integers(1, 9))
        if b + 2 <= k:
            edges.append([b, b + 2, x, 0, {0: x}])
        g = dict(V=V, edges=edges, vw=[0.0] + [float(rng.integers(5, 40)) for _ in range(V - 2)] + [0.0], phasing=[([1, 2, 3], 3)] if r % 3 == 0 else [], strand="+-."[r % 3])
        out.append(shapes.lay_out(g, rng))
    return out


def second_batch() -> PackedGraphs:
    """the sub-batch of the second parameter set"""
    if "second" not in _CACHE:
        rng = np.random.default_rng(4201)
        hubs, _ = _hub_part(4220, 1, rng)
        dead = shapes.pack(dead_end_graphs(rng), rng, ())
        _CACHE["second"] = PackedGraphs.concat(_synth_part(4210, 8, rng) + [hubs, dead])
    return _CACHE["second"]


def _oracle_pre():
    O = common.oracle_lib()
    O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]; O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
    return O


def raw_part():
    """-> dict(items = [(single-graph PackedGraphs, phases, distance)] as add_raw / emu_run_raw take them, staged = the oracle's pre-steps'
    output of every item they pass, ok[n] = passed?, folded[n] = boundaries the oracle folded, dropped[n] = distinct phases it dropped)"""
    if "raw" in _CACHE:
        return _CACHE["raw"]
    O = _oracle_pre(); rng = np.random.default_rng(4301)
    items = []
    for t in range(30):
        g, phases = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 9)), strand="+-."[t % 3])
        if t % 4 == 0:
            phases = phases + phases[:2]                              # duplicate phases: equal lists fold their counts
        pg = PackedGraphs.from_graphs([g])
        pg.edge_rank = np.array(sorted(range(len(g["edges"])), key=lambda k: (g["edges"][k][0], g["edges"][k][1])), np.int32)
        pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
        items.append((pg, phases, int((10000, 150, 0)[t % 3])))
    staged_batch()
    n_hubs = 0
    for g in _CACHE["hub_graphs"][::5]:
        ends = [(e[0], e[1]) for e in g["edges"] if e[0] == 0 or e[1] == g["V"] - 1]
        if len(set(ends)) != len(ends):                               # (the raw entry point refuses parallel edges at the source / sink)
            continue
        pg, phases = shapes.raw_form(g)
        items.append((pg, phases, 10000)); n_hubs += 1
        if n_hubs == 12: break
    staged, ok, folded, dropped = [], [], [], []
    for pg, phases, dist in items:
        want, sm, tm, rc = A.pre_assemble(pg, phases, dist, _lib=O, _prefix="ora")
        ok.append(rc == 0)
        if rc == 0:
            staged.append(want); folded.append(len(sm) + len(tm))
            dropped.append(len(set(tuple(co) for co, _ in phases)) - int(want.g_np[0]))
        else:
            folded.append(0); dropped.append(0)
    _CACHE["raw"] = dict(items=items, staged=PackedGraphs.concat(staged), ok=np.array(ok), folded=np.array(folded), dropped=np.array(dropped), n_hubs=n_hubs)
    return _CACHE["raw"]


def oracle_of(part: str):
    """the oracle's answer for a part ("staged" | "second" under its parameters | "raw" = the staged graphs of the raw part, default parameters;
    "raw2" = the same under the second set), computed once -> dict(pg, params, res, iters, traces, census)"""
    key = "oracle_" + part
    if key not in _CACHE:
        pg = staged_batch() if part == "staged" else second_batch() if part == "second" else raw_part()["staged"]
        prm = second_params() if part in ("second", "raw2") else None
        res, st, _, traces = common.oracle_run(pg, threads=THREADS, trace=True, params=prm)
        _, _, per_graph = shapes.census_of(pg, threads=THREADS, params=prm)
        _CACHE[key] = dict(pg=pg, params=prm, res=res, iters=st[:, 3].copy(), traces=traces, census=per_graph, total_edge_ids=st[:, 2].copy())
    return _CACHE[key]


def expected_classes(part: str, first: int):
    """the class every graph of a part ends in when pick_class starts at `first`: that class, or the class the graph's size asks for where
    that one is larger (the mix reaches 60 vertices, class 0 holds 32: such a graph runs in class 1 whatever smaller class comes first) --
    the size's class as the emulation's host policy finds it without a first class"""
    key = "natural_" + part
    if key not in _CACHE:
        if part in ("raw", "raw2"):
            _CACHE[key] = common.emu_run_raw(raw_part()["items"], full=True)[2]
        else:
            _CACHE[key] = common.emu_run(staged_batch() if part == "staged" else second_batch())[2]
        assert _CACHE[key].max() <= 1 and (_CACHE[key] == 0).sum() >= 20, _CACHE[key]      # the class-0 kernel gets its share of the mix
    return np.maximum(_CACHE[key], first)


OP_NAMES = {1: "broken", 2: "trivial fast", 3: "trivial now", 4: "trivial best", 5: "small now", 6: "smallest", 7: "unsplit now", 8: "unsplit best", 9: "greedy", 10: "collect"}


def census():
    """name -> events, every line counted in the oracle over the three parts"""
    if "census" in _CACHE:
        return _CACHE["census"]
    out = {"op %d %s" % (c, OP_NAMES[c]): 0 for c in range(1, 11)}
    for name in ("router, phasing lists", "router, no phasing lists", "router, one sample", "router, several samples"):
        out[name] = 0
    for fb in ("2", "3", "4", "5-8"):
        for d in ("in", "out"):
            out["fan %s %s" % (fb, d)] = 0
    K = shapes.kernel_constants()
    for part in ("staged", "second", "raw"):
        o = oracle_of(part)
        for t in o["traces"]:
            for ev in t:
                if 1 <= ev[0] <= 10: out["op %d %s" % (ev[0], OP_NAMES[ev[0]])] += 1
        for cen in o["census"]:
            for key, n in cen.items():
                if key[0] == 0:
                    fb = shapes.fan_bucket(key[2], K)
                    if fb in ("2", "3", "4", "5-8"): out["fan %s %s" % (fb, "out" if key[1] == 0 else "in")] += n
                else:
                    out["router, phasing lists" if key[3] else "router, no phasing lists"] += n
                    out["router, one sample" if key[4] else "router, several samples"] += n
    raw = raw_part()
    out["raw graphs with a folded boundary"] = int((raw["folded"] > 0).sum())
    out["raw graphs with a dropped phase"] = int((raw["dropped"] > 0).sum())
    _CACHE["census"] = out
    return out


def census_table() -> str:
    return "\n".join("%-40s %6d" % kv for kv in census().items())


def forced_hub_census(K):
    """the shapes.Census of the mix's graphs as the group of classes 10 / 13 sees them (every graph of the mix runs there under force_class)"""
    cen = None
    for part in ("staged", "second"):
        o = oracle_of(part)
        c = shapes.Census(o["census"], np.full(o["pg"].n, 10, np.int32), o["pg"].g_nv, K)
        cen = c if cen is None else cen.add(c)
    return cen


def natural_size_batch() -> PackedGraphs:
    """two graphs each of the natural size of classes 9, 10 and 13 with the features on (phasing paths, samples, strands, touching exons):
    NC > 16 chunks per sweep and long lists, which no small graph forced into a class reaches"""
    if "natural" not in _CACHE:
        kw = dict(n_graphs=2, phasing_per_graph=40, n_samples=3, strand_mode=1, layout_mode=1)
        _CACHE["natural"] = PackedGraphs.concat([A.synth(seed=201, v_min=900, v_max=1000, edges_per_vertex=4, weight_mode=2, **kw),
                                                 A.synth(seed=202, v_min=1200, v_max=1500, edges_per_vertex=3, weight_mode=2, **kw),
                                                 A.synth(seed=203, v_min=2500, v_max=2500, edges_per_vertex=3, weight_mode=1, **kw)])
    return _CACHE["natural"]


NATURAL_CLASSES = (9, 9, 10, 10, 13, 13)


def large_raw_items(n: int = 3, seed: int = 4401):
    """raw graphs of class-10 size (gene_like_raw of 520 runs, V around 1300) that pass the oracle's pre-steps -> (items, the oracle's staged graphs)"""
    if "large_raw" not in _CACHE:
        O = _oracle_pre(); rng = np.random.default_rng(seed); items = []; staged = []
        while len(items) < n:
            g, phases = common.gene_like_raw(rng, n_runs=520, strand="+-."[len(items) % 3])
            pg = PackedGraphs.from_graphs([g])
            pg.edge_rank = np.array(sorted(range(len(g["edges"])), key=lambda k: (g["edges"][k][0], g["edges"][k][1])), np.int32)
            want, _, _, rc = A.pre_assemble(pg, phases, 10000, _lib=O, _prefix="ora")
            if rc == 0:
                items.append((pg, phases, 10000)); staged.append(want)
        _CACHE["large_raw"] = (items, PackedGraphs.concat(staged))
    return _CACHE["large_raw"]


# the id-width pair: class-13 graphs whose creation ids end on either side of 65 535 (the oracle's total_edge_ids: 74 476 and 61 098)
ID_WIDTH_PAIR = (dict(seed=302, n_graphs=1, v_min=3800, v_max=3800, edges_per_vertex=6), dict(seed=302, n_graphs=1, v_min=2800, v_max=2800, edges_per_vertex=8))


def id_width_batch() -> PackedGraphs:
    if "idw" not in _CACHE:
        _CACHE["idw"] = PackedGraphs.concat([A.synth(**kw) for kw in ID_WIDTH_PAIR])
    return _CACHE["idw"]
