"""The batches of tests/test_turn_handover_cpu.py and tests/test_turn_handover_gpu.py (and tools/turn_handover_parity.py): the hand-over between
the trivial-vertex sweep and the smallest-edge sweep -- the removal of a smallest edge followed by the evaluation of its two endpoints alone
(sweep_smallest_body) and the trivial-vertex scan that is skipped after the star of a sweep's only candidate (sweep_trivial_body).

Nothing here looks into the kernel.  What a batch exercises is read off the ORACLE's op trace and the graphs as they were packed (the
coverage tests of tests/test_turn_handover_cpu.py); both tiers then compare records, iteration counts and the whole op trace with the oracle, tolerance 0.

The hand-made graphs are layered: the source reaches every vertex of the first layer by TWO parallel edges, consecutive layers are fully
connected, every vertex of the last layer reaches the sink by two parallel edges.  Every inner vertex then has two or more edges on both
sides, no vertex is trivial, and the first rule that fires is the smallest-edge rule on the edge whose weight was made small: which edge was
removed, where it stood in its two lists and what the degrees were is known from the packed graph and the first trace event alone."""
import numpy as np

import aletsch_amd as A
from aletsch_amd.packed import PackedGraphs
import common
import device_run as DR
import shapes

TRACE_CAP = 1 << 13
OP_BROKEN, OP_TRIVIAL_FAST, OP_TRIVIAL_NOW, OP_TRIVIAL_BEST, OP_SMALL_NOW, OP_SMALLEST = 1, 2, 3, 4, 5, 6
_CACHE = {}


def layered(widths, w=10.0, tweak=(), extra=(), splice=(), phasing=(), strand=0):
    """tweak: ((s, t, k), weight) sets the weight of the k-th edge s -> t; extra: further edges (s, t, weight); splice: ((s, t), w_in, w_out)
    puts a NEW vertex on the edge s -> t, which takes the index t (t and every later vertex move up by one: a later splice and the phasing
    lists count in the new numbering); phasing: (vertex list, count)"""
    V = 2 + sum(widths); layers = []; k = 1
    for n in widths:
        layers.append(list(range(k, k + n))); k += n
    E = []
    mk = lambda s, t, ww: [s, t, float(ww), strand, {0: float(ww)}]
    for x in layers[0]:
        E += [mk(0, x, w), mk(0, x, w)]
    for a, b in zip(layers, layers[1:]):
        E += [mk(x, y, w) for x in a for y in b]
    for x in layers[-1]:
        E += [mk(x, V - 1, w), mk(x, V - 1, w)]
    for (s, t, kk), ww in tweak:
        m = [e for e in E if e[0] == s and e[1] == t][kk]; m[2] = float(ww); m[4] = {0: float(ww)}
    E += [mk(s, t, ww) for s, t, ww in extra]
    g = dict(V=V, edges=E, vw=[0.0] * V, phasing=[], strand="." if strand == 0 else "+")
    for (s, t), w_in, w_out in splice:
        g = shapes.open_room(g, t, 1)
        old = [e for e in g["edges"] if e[0] == s and e[1] == t + 1][0]; g["edges"].remove(old)
        g["edges"] += [mk(s, t, w_in), mk(t, t + 1, w_out)]
    g["phasing"] = [(list(v), int(c)) for v, c in phasing]
    return g


def handmade():
    """-> [(name, graph dict)]: one case of the removal each (layers (3, 3): vertices 1..3 and 4..6, sink 7)"""
    return [
        ("head", layered((3, 3), tweak=[((1, 4, 0), 0.5)])),                        # first of 1's out-list and of 4's in-list
        ("middle", layered((3, 3), tweak=[((2, 5, 0), 0.5)])),
        ("tail", layered((3, 3), tweak=[((3, 6, 0), 0.5)])),
        ("leaves_source", layered((2, 2), tweak=[((0, 1, 0), 0.5)])),               # out(source) is a counted list
        ("enters_sink", layered((2, 2), tweak=[((4, 5, 1), 0.5)])),                 # in(sink) is a counted list
        ("out_deg_to_1", layered((3, 2), tweak=[((1, 4, 0), 0.5)])),                # out_deg[1]: 2 -> 1
        ("in_deg_to_1", layered((2, 3), tweak=[((1, 3, 0), 0.5)])),                 # in_deg[3]: 2 -> 1
        ("parallel", layered((3, 3), extra=[(2, 5, 0.5)])),                         # two edges 2 -> 5, the second one small
        ("back_to_the_other_end", layered((3, 3), tweak=[((1, 4, 0), 0.25)], extra=[(1, 4, 0.5)])),   # once 1 -> 4 is gone the smallest edge of 1 AND of 4 is its twin
        ("two_hits", layered((3, 3), tweak=[((1, 4, 0), 0.05), ((2, 6, 0), 0.04)])),     # ratio < 0.01 twice in one sweep
    ]


def dominate_flip():
    """The star of the only candidate makes ANOTHER vertex type 1 through the phasing lists alone.  Vertex 3 (one edge in, 1 -> 3; two out, to 4 and
    5: a star of two, which does not take the vertex's own last edge away through the removal that raises the flag) is the one candidate.  Vertex 6 has the single in-edge 4 -> 6, vertex 4 has other edges out, and 4 -> 6 lies on the phasing path [1, 3, 4, 6],
    which ENDS on it, and on [3, 4, 6, 7], which goes on past it: the second does not dominate the first while their prefixes differ
    (3 -> 4 preceded by 1 -> 3 in the one, by nothing in the other), so vertex 6 is of type 2.  The star of 3 merges 1 -> 3 -> 4 into 1 -> 4 (and 1 -> 3 -> 5 into 1 -> 5):
    the first path becomes [1, 4, 6], the second [1, 4, 6, 7], the prefixes agree, 4 -> 6 is dominated and vertex 6 is of type 1.  No degree
    falls to <= 1 on the way, not even in passing: vertex 1 has three edges out, vertices 4 and 5 three and four edges in.
    Where the early clear happens: on the device, whose first scan meets the dominate queries of vertices 3 and 6 in its first chunk, has them
    answered, starts again at vertex 1 and then counts one candidate in the whole graph.  In the single-lane emulation a chunk is ONE vertex, so a
    dominate query beyond vertex 1 always leaves a scan that did not start at vertex 1: no count, no clear -- there the case pins the count's
    validity rule, like need_in_second_chunk()."""
    w = 10.0
    mk = lambda s, t, ww=w: [s, t, float(ww), 0, {0: float(ww)}]
    E = [mk(0, 1), mk(0, 1), mk(0, 2), mk(0, 2),
         mk(1, 3), mk(1, 4), mk(1, 5), mk(2, 4), mk(2, 5),
         mk(3, 4, 6.0), mk(3, 5, 6.0),
         mk(4, 5), mk(4, 6), mk(4, 7),
         mk(5, 7), mk(5, 8),
         mk(6, 7, 5.5), mk(6, 8, 5.5),               # balance ratio 11 / 10, better than vertex 3's 12 / 10: were 6 of type 1 from the start, it would go first
         mk(7, 9), mk(7, 9), mk(8, 9), mk(8, 9)]
    return dict(V=10, edges=E, vw=[0.0] * 10, phasing=[([1, 3, 4, 6], 4), ([3, 4, 6, 7], 3)], strand=".")


def need_in_second_chunk():
    """23 layers of three vertices, a candidate spliced in at vertex 4 and another at vertex 68, whose in-edge 65 -> 68 lies on a phasing path
    while 65 has other edges out: the scan that starts at vertex 1 leaves the second chunk with a dominate query, the scan that finishes
    the sweep starts at vertex 64 and sees ONE candidate of two.  Its count must not stand for the graph: the best candidate is vertex 4, whose
    star touches no phasing path and no degree below 3, so nothing would raise the flag again for vertex 68."""
    return layered((3,) * 23, splice=[((1, 4), 10.0, 11.0), ((65, 68), 10.0, 12.0)], phasing=[([65, 68, 69], 4)])


def trivial_cases():
    """-> [(name, graph dict, parameters or None)]: the scan after a star (layers (2, 2): vertices 1, 2 and 3, 4 before the splices)"""
    p15 = A.default_params(); p15.max_decompose_error_ratio[7] = 1.5
    return [
        ("dominate_flip", dominate_flip(), None),
        ("need_in_second_chunk", need_in_second_chunk(), None),
        ("one_candidate", layered((2, 2), splice=[((1, 3), 10.0, 12.0)]), None),                          # its star leaves no candidate: the next scan is the skipped one
        ("two_candidates", layered((2, 2), splice=[((1, 3), 10.0, 12.0), ((2, 5), 10.0, 13.0)]), None),    # the first scan counts two: the flag stays
        ("phasing_need", layered((2, 2), splice=[((1, 3), 10.0, 12.0)], phasing=[([1, 3, 4], 4)]), None),  # the candidate's edge lies on a phasing path and its far end has other edges: dominate query, then hs_replace in the star
        ("phasing_two", layered((2, 2), splice=[((1, 3), 10.0, 12.0), ((2, 5), 10.0, 13.0)], phasing=[([1, 3, 4], 4), ([2, 5, 6], 3)]), None),
        ("jump_above_one", layered((2, 2), splice=[((1, 3), 10.0, 12.0)]), p15),                          # stage 0 runs: that sweep is not the skippable one
        ("stranded", layered((2, 2), splice=[((1, 3), 10.0, 12.0)], strand=1), None),
    ]


def pack_dicts(graphs, seed=3):
    rng = np.random.default_rng(seed)
    return shapes.pack([shapes.lay_out(g, rng) for g in graphs])


def sorted_edges(g):
    """(s, t) of every edge in creation-id order (shapes.pack sorts by (s, t), stable)"""
    order = sorted(range(len(g["edges"])), key=lambda k: (g["edges"][k][0], g["edges"][k][1]))
    return [(g["edges"][k][0], g["edges"][k][1]) for k in order]


def first_removal(g, trace):
    """the first event of the trace, which must be a smallest-edge removal of an ORIGINAL edge -> dict(code, s, t, place of the edge in s's
    out-list and in t's in-list ("head" / "middle" / "tail" / "only"), the two list lengths before the removal)"""
    code, eid, _, _ = trace[0]
    assert code in (OP_SMALL_NOW, OP_SMALLEST), trace[:3]
    E = sorted_edges(g); s, t = E[eid]
    outl = [k for k, (a, b) in enumerate(E) if a == s]; inl = [k for k, (a, b) in enumerate(E) if b == t]     # (t, id) / (s, id) order == id order here
    place = lambda l: "only" if len(l) == 1 else ("head" if l[0] == eid else ("tail" if l[-1] == eid else "middle"))
    return dict(code=code, eid=eid, s=s, t=t, out_place=place(outl), in_place=place(inl), out_len=len(outl), in_len=len(inl), sink=g["V"] - 1)


def bench_batch():
    if "bench" not in _CACHE:
        _CACHE["bench"] = A.synth(seed=1002, n_graphs=300, v_min=64, v_max=64, fixed_edges=256)
    return _CACHE["bench"]


def small_batch():
    """200 graphs of 32 vertices / 96 edges: class 0, one chunk"""
    if "small" not in _CACHE:
        _CACHE["small"] = A.synth(seed=4001, n_graphs=200, v_min=32, v_max=32, fixed_edges=96)
    return _CACHE["small"]


def far_batch():
    """200 graphs of 100..128 vertices, each with three light edges s -> s + 64 added: source and target of such an edge belong to the same
    lane in two chunks of the sweep.  -> (PackedGraphs, per graph the set of creation ids of the added edges)"""
    if "far" not in _CACHE:
        base = A.synth(seed=4002, n_graphs=200, v_min=100, v_max=128, edges_per_vertex=4)
        rng = np.random.default_rng(4003); graphs = []; marked = []
        for i in range(base.n):
            g = shapes.unpack(base, i); V = g["V"]
            for s in sorted(int(x) for x in rng.choice(np.arange(1, V - 65), size=3, replace=False)):
                w = float(rng.integers(1, 4)) / 8.0
                g["edges"].append([s, s + 64, w, 0, {0: w}])
            graphs.append(g)
            E = sorted_edges(g)
            marked.append({k for k, (a, b) in enumerate(E) if b - a == 64 and 1 <= a and b < V - 1})
        rng = np.random.default_rng(4004)
        _CACHE["far"] = (shapes.pack([shapes.lay_out(g, rng) for g in graphs]), marked)
    return _CACHE["far"]


def fuzz_specs():
    """the fuzz slice: 2 000 graphs of 8..200 vertices, with and without phasing paths and strands"""
    return [dict(seed=4100, n_graphs=500, v_min=8, v_max=200, edges_per_vertex=3),
            dict(seed=4101, n_graphs=500, v_min=8, v_max=200, edges_per_vertex=4, phasing_per_graph=10, weight_mode=2),
            dict(seed=4102, n_graphs=500, v_min=8, v_max=200, edges_per_vertex=3, strand_mode=1, layout_mode=1, weight_mode=1),
            dict(seed=4103, n_graphs=500, v_min=8, v_max=200, edges_per_vertex=3, phasing_per_graph=20, n_samples=3, strand_mode=1, layout_mode=1)]


FUZZ_TRACE_CAP = 1 << 11


def fuzz_part(k):
    if ("fuzz", k) not in _CACHE:
        _CACHE[("fuzz", k)] = A.synth(**fuzz_specs()[k])
    return _CACHE[("fuzz", k)]


def oracle(key, pg, params=None):
    """records, statistics and op traces of a batch, computed once -> dict(res, iters, traces)"""
    k = "oracle_" + key
    if k not in _CACHE:
        res, st, _, tr = common.oracle_run(pg, threads=DR.THREADS, trace=True, params=params)
        _CACHE[k] = dict(res=res, iters=st[:, 3].copy(), traces=tr)
    return _CACHE[k]


def count(traces, code):
    return sum(1 for t in traces for ev in t if ev[0] == code)


def gpu_batches():
    """(name, batch, parameters) of everything the GPU tier runs: batches 1 to 4"""
    out = [("bench", bench_batch(), None), ("small", small_batch(), None), ("far", far_batch()[0], None),
           ("handmade", pack_dicts([g for _, g in handmade()]), None)]
    for name, g, prm in trivial_cases():
        out.append(("trivial_" + name, pack_dicts([g]), prm))
    return out


def bench_raw(stride=3):
    """every stride-th graph of batch 1 as a RAW graph (the pre-steps of assembler::assemble run in the load phase), with the oracle's pre-steps
    applied for the comparison -> (items for add_raw / emu_run_raw, the batch of all items for add_packed_raw, the oracle's staged graphs)"""
    if "raw" not in _CACHE:
        import ctypes as C
        O = common.oracle_lib()
        O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]; O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
        pg = bench_batch(); idx = np.arange(0, pg.n, stride); items = []; staged = []
        for g in idx:
            one = pg.select(np.array([g]))
            want, _, _, rc = A.pre_assemble(one, [], 10000, _lib=O, _prefix="ora")
            assert rc == 0
            items.append((one, [], 10000)); staged.append(want)
        _CACHE["raw"] = (items, pg.select(idx), PackedGraphs.concat(staged))
    return _CACHE["raw"]


# (first class, ALD_DEBUG_TWIN, class): the one-chunk, two-chunk and many-chunk forms of the sweeps and the slab form (7 with the twins on: class 11)
FORCINGS = tuple(DR.forced_kernels((0, 1, 2), twins=(11,))[0])


def mismatches_on_device(name, pg, o, params=None, first=0, twin="0", cls=0, raw=False):
    """the batch with the first class forced, every graph traced, against its cached oracle answer (no graph below the forced class)"""
    r = DR.run(pg, params, first=first, twin=twin, raw=raw, trace_cap=TRACE_CAP)
    tag = f"{name}, first class {first}, twin {twin}" + (", raw" if raw else "")
    return DR.oracle_mismatches(tag, r, o["res"], o["iters"], o["traces"], want_classes=set(range(cls, DR.N_CLASSES)))
