"""Hand-made graphs that END ON ONE OF THE REFERENCE'S ASSERTS -- every way a star, a router, the sweeps and the collect phase can leave a graph
with a status of class ALD_ST_INVARIANT -- and the graphs that must not notice when they run behind one (tests/test_assert_exits_cpu.py,
tests/test_assert_exits_gpu.py, tools/assert_exits_parity.py).

Every graph is seeded, small (4 .. 80 vertices) and accepted by ald_batch_add_packed.  Which assert a graph ends on is never taken from how it
was built: the oracle names the site (oracle/oracle_capi.cc: ora_result_assert_site -- scope + function + tag, the vertex of the rule in flight,
its degrees when the rule began), and the census below is a count over those answers.  Which fail() line of the kernel source raised the status
is the emulation's answer (tests/kernel_emu/emu_capi.cc: emu_result_fail_lines), set against the lines parsed out of decomp_device.h.

The failing star: source -> hub -> k leaves -> sink (out), or its mirror image (in).  The hub's two sides differ by 1 % and every leaf's by
50 %, so that the hub is the one vertex the first sweep decomposes `now` (ratio < 1.02): the star meets its fan edges as they were staged --
the failing edge at a chosen LIST position (the k-th leaf) and, through edge_creation_rank, at a chosen MERGE position, which differ."""
from __future__ import annotations

import os
import re

import numpy as np

import aletsch_amd as A
from aletsch_amd.packed import PackedGraphs
import common
import device_run as DR
import shapes

MIN_EVENTS = 10
K = shapes.kernel_constants()
_CACHE = {}


def params(minw=None, r0=None, r7=None, max_exons=None):
    """None: the defaults; minw: min_guaranteed_edge_weight; r0: the ratio of the smallest-edge rule (0: wide hubs reach the router, shapes.wide_router_params)"""
    if minw is None and r0 is None and r7 is None and max_exons is None: return None
    p = A.default_params()
    if r7 is not None: p.max_decompose_error_ratio[7] = r7
    if max_exons is not None: p.max_num_exons = max_exons
    if minw is not None: p.min_guaranteed_edge_weight = minw
    if r0 is not None: p.max_decompose_error_ratio[0] = r0
    return p


# minwnan: a min_guaranteed_edge_weight that compares with nothing -- the one way a pair weight out of the router fails `w >= min_w - SMIN` (build() raises
# every pair below min_w to min_w, and `w < NaN` raises none); nested: jump_ratio 1.5, under which decompose_vertex_extend tries its new vertices at once
PARAM_SETS = {"default": dict(), "minw2": dict(minw=2.0), "minw0": dict(minw=0.0), "wide": dict(r0=0.0),
              "minwnan": dict(minw=float("nan"), r0=0.0), "nested": dict(minw=0.0, r0=0.0, r7=1.5)}


# ---------------------------------------------------------------------------------------------------------------------------------------
# graph dicts with a creation rank of their own: g["rank"][i] is the rank of g["edges"][i] (None: the order of g["edges"])
# ---------------------------------------------------------------------------------------------------------------------------------------
def mirror(g: dict) -> dict:
    m = shapes.mirror(g)
    m["rank"] = None if g.get("rank") is None else list(g["rank"])
    for key in ("lpos", "rpos"):
        if key in g: m.pop(key, None)
    return m


def pack(graphs) -> PackedGraphs:
    """shapes.pack with the creation ranks the graphs carry: the CSR order is (source, target, position in g["edges"]), the rank is whatever
    g["rank"] says, compacted to a permutation"""
    out = []; ranks = []; counts = []; any_count = any(g.get("count") is not None for g in graphs)
    for g in graphs:
        E = len(g["edges"]); order = sorted(range(E), key=lambda k: (g["edges"][k][0], g["edges"][k][1]))
        edges = [tuple(g["edges"][k]) for k in order]
        out.append(dict(g, edges=edges))
        r = list(range(E)) if g.get("rank") is None else list(g["rank"])
        assert sorted(r) == list(range(E)), "the creation rank is a permutation"
        ranks.append(np.array([r[k] for k in order], np.int32))
        cnt = g.get("count")
        counts.append(np.array([len(e[4]) for e in edges] if cnt is None else [cnt[k] for k in order], np.int32))
    pg = PackedGraphs.from_graphs(out)
    pg.edge_rank = np.concatenate(ranks).astype(np.int32) if ranks else np.zeros(0, np.int32)
    if any_count: pg.edge_count = np.concatenate(counts).astype(np.int32)
    return pg


# ---------------------------------------------------------------------------------------------------------------------------------------
# stars
# ---------------------------------------------------------------------------------------------------------------------------------------
STAR_FANS = tuple(sorted(set((1, 2, 3, 4, 5, 6, 7, 8, 9, 16, K["STAR_MAX"] - 1, K["STAR_MAX"], K["STAR_MAX"] + 1, 48, 63, 64, 65, 70)
                             + tuple(x + d for x in set(K["STARFIX_MAX"]) for d in (-1, 0, 1)))))


def _positions(k):
    """first, a middle and the last position of a fan of k"""
    return sorted(set((0, k // 2, k - 1)))


def fail_star(rng, k, out, items, minw=0.01, centre=None, samples=None, leaf_ratio=1.5, hub_ratio=1.01):
    """source -> hub -> k leaves -> sink.  items: [(what, list position, merge position)], what in
         "count"   the fan edge at that list position has edge_info.count == 0
         "weight"  that fan edge weighs less than min_guaranteed_edge_weight - SMIN
       and the fan edge at list position p is the q-th of the fan in creation order (merge position q); the other fan edges take the remaining
       merge positions in a seeded random order.  centre: None | "count" | "weight" -- the same for the hub's one edge on the narrow side.
       samples: None (sample 0 on every edge) or a function (kind, j) -> {sample: abundance} for kind in "centre", "fan", "leaf"."""
    V = k + 3; hub = 1; sink = V - 1
    fw = [float(x) for x in (minw * (3.0 + 20.0 * rng.random(k)))]
    fixed = {}
    for what, p, q in items:
        assert 0 <= p < k and 0 <= q < k and p not in fixed and q not in fixed.values()
        fixed[p] = q
        if what == "weight": fw[p] = minw * 0.5
    cw = float(sum(fw)) * hub_ratio
    if centre == "weight": cw = minw * 0.5
    sp = samples if samples is not None else (lambda kind, j: {0: 1.0 + j})
    edges = [[0, hub, cw, 0, sp("centre", 0)]]
    for j in range(k): edges.append([hub, 2 + j, fw[j], 0, sp("fan", j)])
    for j in range(k): edges.append([2 + j, sink, fw[j] * leaf_ratio, 0, sp("leaf", j)])
    count = [len(e[4]) for e in edges]
    for what, p, q in items:
        if what == "count": count[1 + p] = 0
    if centre == "count": count[0] = 0
    # creation ranks: the fan's merge order is chosen, where the fan's ids lie among the others' is drawn
    free = [q for q in range(k) if q not in fixed.values()]; rng.shuffle(free)
    merge_pos = [fixed[p] if p in fixed else free.pop() for p in range(k)]
    E = len(edges); slots = sorted(int(x) for x in rng.choice(E, size=k, replace=False)); others = [r for r in range(E) if r not in set(slots)]; rng.shuffle(others)
    rank = [0] * E
    for p in range(k): rank[1 + p] = slots[merge_pos[p]]
    for i in [0] + list(range(1 + k, E)): rank[i] = others.pop()
    g = dict(V=V, edges=edges, vw=[0.0] + [float(rng.integers(1, 40)) for _ in range(V - 2)] + [0.0], phasing=[], strand=".", count=count, rank=rank)
    if not out: g = mirror(g)
    return shapes.lay_out(g, rng)


def star_cases(fans=STAR_FANS, without=()):
    """[(label, parameter set, graph)] -- every way a star can end, per fan size and direction; without: labels left out (the census's self-check)"""
    rng = np.random.default_rng(6101); out = []
    add = lambda label, ps, g: out.append((label, ps, g)) if label not in without else None
    for k in fans:
        for d in (True, False):
            pos = _positions(k); reps = {1: 6, 2: 3}.get(len(pos), 1)          # (a fan of 1 or 2 has fewer positions: more draws, so that a line holds its 10 events)
            for ps, minw in (("default", 0.01), ("minw2", 2.0)):
                # one failing fan edge: list position x merge position, first / middle / last each
                for rep in range(reps):
                    for p in pos:
                        for q in pos:
                            add("star count", ps, fail_star(rng, k, d, [("count", p, q)], minw))
                            add("star weight", ps, fail_star(rng, k, d, [("weight", p, q)], minw))
                for rep in range(5):
                    add("star centre count", ps, fail_star(rng, k, d, [], minw, centre="count"))
                    add("star centre weight", ps, fail_star(rng, k, d, [], minw, centre="weight"))
                if k >= 2:
                    # two failing fan edges whose merge order and list order disagree; a zero count and an under-weight edge in one star
                    a, b = pos[0], pos[-1]
                    add("star two counts", ps, fail_star(rng, k, d, [("count", a, b), ("count", b, a)], minw))
                    add("star count and weight", ps, fail_star(rng, k, d, [("count", a, a), ("weight", b, b)], minw))
                    add("star count and weight", ps, fail_star(rng, k, d, [("weight", a, b), ("count", b, a)], minw))
                    add("star count and weight", ps, fail_star(rng, k, d, [("count", a, b)], minw, centre="weight"))
                    add("star count and weight", ps, fail_star(rng, k, d, [("weight", b, a)], minw, centre="count"))
    return out


def extreme_star(rng, k, out, kind):
    """Stars whose weights leave the range the balance step keeps in order -- staging accepts any double, and with min_guaranteed_edge_weight
    == 0 nothing is raised to a minimum:
      "consumed"   the last fan edges in merge order weigh SMIN each: once the heavy ones are merged, what is left of the centre equals the next
                   pair weight within SMIN, so that merge uses the centre up while fan edges are left -- merge_adjacent_edges returns -1 for
                   them (scallop.cc:2397) and decompose_vertex_replace ends on assert(gr.degree(root) == 0) (scallop.cc:2139)
      "remainder"  weights around 1e20: the rounding error of the centre's running remainder exceeds SMIN, the last merge leaves a piece of it
      "nan"        weights of 1e200 and one of 0: sqrt(w_in * w_out) overflows, 0 * inf is a NaN pair weight, which fails `w >= min_w - SMIN`
                   (the leaf behind the weightless edge has a second edge on that side, so that its own weight sums stay above SMIN).  A fan
                   that comes IN takes min(fan, centre) with the fan first: the NaN loses, every pair weight is inf, and the star ends as
      "overflow"   does: weights of 1e200, every pair weight inf -- split_edge cuts a piece of weight inf off an edge of weight inf, and
                   merge_adjacent_equal_edges asserts on fabs(inf - inf), a NaN (scallop.cc:2242-2378); "overflow count": with an uncounted fan edge"""
    V = k + 3; hub = 1; sink = V - 1; extra = []; last = []
    if kind == "consumed":
        assert k >= 3
        fw = [float(x) for x in (1.0 + 9.0 * rng.random(k))]
        last = [int(j) for j in rng.choice(k, size=int(rng.integers(2, min(k - 1, 4) + 1)), replace=False)]
        for j in last: fw[j] = 1e-5
        cw = sum(fw) * 0.99                     # (the balance step scales the fan down: 0.995e-5 a piece)
    elif kind == "remainder":
        fw = [float(x) for x in (1e20 * (1.0 + 9.0 * rng.random(k)))]; cw = sum(fw) * 1.01
    elif kind.startswith("overflow"):
        fw = [float(x) for x in (1e200 * (1.0 + rng.random(k)))]; cw = sum(fw) * 1.01
    else:
        fw = [float(x) for x in (1e200 * (1.0 + rng.random(k)))]; z = int(rng.integers(0, k)); fw[z] = 0.0; cw = sum(fw) * 1.01
        extra = [[0, 2 + z, 1.0, 0, {0: 1.0}]]
    edges = [[0, hub, cw, 0, {0: 1.0}]]
    for j in range(k): edges.append([hub, 2 + j, fw[j], 0, {0: 1.0 + j}])
    for j in range(k): edges.append([2 + j, sink, (fw[j] if fw[j] > 0 else 1.0) * 1.5, 0, {0: 2.0}])
    edges += extra
    E = len(edges); rank = [int(x) for x in rng.permutation(E)]
    if last:                                    # the light fan edges are the newest of the fan
        fan_ranks = sorted(rank[1 + j] for j in range(k)); heavy = [j for j in range(k) if j not in last]; rng.shuffle(heavy)
        for q, j in enumerate(heavy + last): rank[1 + j] = fan_ranks[q]
    count = None
    if kind == "overflow count":                # ... and a fan edge that is not counted: the infinite pair weight in front of it (or at it) is met first
        count = [1] * E; count[1 + int(rng.integers(0, k))] = 0
    g = dict(V=V, edges=edges, vw=[0.0] + [float(rng.integers(1, 40)) for _ in range(V - 2)] + [0.0], phasing=[], strand=".", count=count, rank=rank)
    if not out: g = mirror(g)
    return shapes.lay_out(g, rng)


def extreme_star_cases(fans=STAR_FANS, without=()):
    rng = np.random.default_rng(6102); out = []
    for k in fans:
        for d in (True, False):
            for kind in ("consumed", "remainder", "nan", "overflow", "overflow count"):
                if "star " + kind in without or (kind == "consumed" and k < 3) or (k < 2 and not kind.startswith("overflow")): continue
                for r in range(24 if (kind == "remainder" and k <= 4) else 12): out.append(("star " + kind, "minw0", extreme_star(rng, k, d, kind)))
    return out


def late_count_star(rng, k, out, depth):
    """a star whose merges all go through, but one of them leaves an edge with an EMPTY sample intersection (a count of 0 is no assert where it is
    computed): the assert is met when that edge is merged AGAIN, by a later rule.  depth 1: the hub's own merge empties it (centre {1, 2} x fan
    {3}), the leaf behind asserts; depth 2: the hub leaves {2} ({1, 2} x {2, 3}), the first leaf empties it ({2} x {3}), the second asserts."""
    V = 2 + 1 + k * depth + 1; hub = 1; sink = V - 1
    fw = [float(x) for x in (3.0 + 20.0 * rng.random(k))]; cw = sum(fw) * 1.01
    bad = int(rng.integers(0, k)); ok = {1: 2.0, 2: 2.0}
    edges = [[0, hub, cw, 0, {1: 4.0, 2: 5.0}]]
    for j in range(k):
        v = 2 + j * depth
        chain = ([{3: 2.0}, ok] if depth == 1 else [{2: 3.0, 3: 1.0}, {3: 2.0}, ok]) if j == bad else [ok] * (depth + 1)
        edges.append([hub, v, fw[j], 0, dict(chain[0])])
        for q in range(1, depth + 1):
            edges.append([v + q - 1, sink if q == depth else v + q, fw[j] * (1.5 ** q), 0, dict(chain[q])])
    g = dict(V=V, edges=edges, vw=[0.0] + [float(rng.integers(1, 40)) for _ in range(V - 2)] + [0.0], phasing=[], strand=".", count=None,
             rank=[int(x) for x in rng.permutation(len(edges))])
    if not out: g = mirror(g)
    return shapes.lay_out(g, rng)


def late_count_cases(without=()):
    rng = np.random.default_rng(6103); out = []
    if "late count" in without: return out
    for k in (2, 3, 4, 5, 8, 16, K["STAR_MAX"], K["STAR_MAX"] + 1):
        for d in (True, False):
            for depth in (1, 2):
                for r in range(2): out.append(("late count", "default", late_count_star(rng, k, d, depth)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# routers
# ---------------------------------------------------------------------------------------------------------------------------------------
def hub(rng, kin, kout, routes=(), in_samples=None, out_samples=None, in_strand=None, out_strand=None, w=6.0, in_pre=None):
    """source -> a_i -> hub -> b_j -> sink with tied weights (every feeder and receiver is a trivial vertex of ratio 1.0: the first sweep merges
    them away, and the hub is left with kin edges from the source and kout edges to the sink, each carrying the INTERSECTION of the sample sets
    of the two edges it was merged from).  routes: (i, j, count) phasing paths a_i -> hub -> b_j.  in_pre[i]: sample set of source -> a_i when
    it differs from that of a_i -> hub (an empty intersection leaves a hub edge with count 0 without any assert)."""
    V = kin + kout + 3; hubv = 1 + kin; sink = V - 1
    one = {0: 5.0}
    ins = [dict(one) for _ in range(kin)] if in_samples is None else [dict(x) for x in in_samples]
    outs = [dict(one) for _ in range(kout)] if out_samples is None else [dict(x) for x in out_samples]
    pre = [dict(x) for x in ins] if in_pre is None else [dict(ins[i]) if in_pre[i] is None else dict(in_pre[i]) for i in range(kin)]
    wi, wo = w * kout, w * kin
    edges = []
    for i in range(kin): edges.append([0, 1 + i, wi, 0, pre[i]])
    for i in range(kin): edges.append([1 + i, hubv, wi, 0 if in_strand is None else in_strand[i], ins[i]])
    for j in range(kout): edges.append([hubv, hubv + 1 + j, wo, 0 if out_strand is None else out_strand[j], outs[j]])
    for j in range(kout): edges.append([hubv + 1 + j, sink, wo, 0, dict(outs[j])])
    g = dict(V=V, edges=edges, vw=[0.0] + [float(rng.integers(1, 40)) for _ in range(V - 2)] + [0.0],
             phasing=[([1 + i, hubv, hubv + 1 + j], c) for i, j, c in routes], strand=".", count=None, rank=[int(x) for x in rng.permutation(len(edges))])
    return shapes.lay_out(g, rng)


def router_sizes():
    """2 + 2, the small form up to its largest size, the smallest large one, LP - 1 / LP / LP + 1, and the largest that fits 80 vertices (the small
    form ends where the header says: at LP or at its arena limit, whichever comes first)"""
    LP = K["LP"]; top = max(n for n in range(4, LP + 1) if K["router_small"](n // 2, n - n // 2, False))
    sizes = [(2, 2), (2, 3), (3, 3), (4, 5), (top // 2, top - top // 2), ((top + 1) // 2, top + 1 - (top + 1) // 2)]
    sizes += [(n // 2, n - n // 2) for n in (LP - 1, LP, LP + 1)] + [(20, 20), (35, 35)]
    return sorted(set(sizes))


def router_cases(without=()):
    rng = np.random.default_rng(6104); out = []
    add = lambda label, g: out.append((label, "wide", g)) if label not in without else None
    S1, S2 = {1: 5.0}, {2: 5.0}
    for kin, kout in router_sizes():
        for r in range(12 if (kin, kout) == (2, 2) else 6):
            some_routes = [(int(rng.integers(0, kin)), int(rng.integers(0, kout)), int(rng.integers(2, 9))) for _ in range(1 + r)] if r % 2 else []
            # mixed strand: strands 1 and 2 on one side of the hub (router.cc:71-76)
            st = [1 + (i + r) % 2 for i in range(kin)]
            add("router strand", hub(rng, kin, kout, routes=some_routes, in_strand=st))
            st = [1 + (j + r) % 2 for j in range(kout)]
            add("router strand", hub(rng, kin, kout, routes=some_routes, out_strand=st))
            # no routes, no shared sample: an isolated node finds no partner -> UGraph::add_edge out of range (left side first, then right)
            add("router no partner", hub(rng, kin, kout, in_samples=[S1] * kin, out_samples=[S2] * kout))
            add("router no partner", hub(rng, kin, kout, in_samples=[S1] * kin, out_samples=[S1] * (kout - 1) + [S2]))
            # a hub edge of count 0 (empty intersection of the two edges it was merged from) that no route covers: a node without an edge
            z = int(rng.integers(0, kin))
            add("router bare node", hub(rng, kin, kout, in_pre=[S2 if i == z else None for i in range(kin)], in_samples=[S1] * kin, out_samples=[S1] * kout))
            # ... covered by every route there is: the decomposition behind the router meets it (both ends of the pair have two pairs or more)
            full = [(i, j, 2 + (i + j) % 3) for i in range(kin) for j in range(kout)] if kin * kout <= 450 else None
            if full is not None:
                add("router count", hub(rng, kin, kout, routes=full, in_pre=[S2 if i == z else None for i in range(kin)], in_samples=[S1] * kin, out_samples=[S1] * kout))
                # ... or edges that are counted but share no sample: the new edge between them has an empty set
                add("router empty pair", hub(rng, kin, kout, routes=full, in_samples=[S1] * kin, out_samples=[S2 if j == z % kout else S1 for j in range(kout)]))
    return out


def bare_hub(rng, kin, kout, win=None, wout=None):
    """source => hub => sink: kin parallel edges in, kout parallel edges out, nothing else -- no trivial vertex, so the router is the first rule to fire"""
    win = [6.0 * kout] * kin if win is None else win; wout = [6.0 * kin] * kout if wout is None else wout
    edges = [[0, 1, w, 0, {0: 5.0}] for w in win] + [[1, 2, w, 0, {0: 5.0}] for w in wout]
    g = dict(V=3, edges=edges, vw=[0.0, float(rng.integers(1, 40)), 0.0], phasing=[], strand=".", count=None, rank=[int(x) for x in rng.permutation(len(edges))])
    return shapes.lay_out(g, rng)


def nested_hub(rng, r):
    """source -> a -> hub (2 in, 2 out) under jump_ratio 1.5: a is a vertex no rule may touch (in-edge of strand 1, out-edge of strand 2) and its
    edge into the hub weighs less than SMIN (kept from the smallest-edge rule by a's single out-edge).  The router splits the hub, that edge gets
    a vertex of its own (its larger sample abundance makes it the partner of the second out-edge, so it has two pairs), and
    resolve_single_trivial_vertex meets a weight sum below SMIN there"""
    tiny = float(2e-6 + 1e-6 * (r % 5)); big = float(4 + r % 7)
    edges = [[0, 1, 5.0, 1, {0: 5.0}], [1, 2, tiny, 2, {0: 50.0}], [0, 2, big, 0, {0: 5.0}], [2, 3, big / 2, 0, {0: 5.0}], [2, 3, big / 2 + 1.0, 0, {0: 5.0}]]
    g = dict(V=4, edges=edges, vw=[0.0, 3.0, float(rng.integers(1, 40)), 0.0], phasing=[], strand=".", count=None, rank=[int(x) for x in rng.permutation(len(edges))])
    return shapes.lay_out(g, rng)


def router_param_cases(without=()):
    rng = np.random.default_rng(6110); out = []
    for r in range(12):
        kin, kout = ((2, 2), (2, 3), (3, 3), (7, 7))[r % 4]
        if "router pair weight" not in without: out.append(("router pair weight", "minwnan", bare_hub(rng, kin, kout)))
        if "router nested" not in without: out.append(("router nested", "nested", nested_hub(rng, r)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the sweeps and the late exits
# ---------------------------------------------------------------------------------------------------------------------------------------
SWEEP_AT = (1, 63, 64, 65, 71)                # lane 1 of the first chunk, its last lane, lane 0 / 1 of the second chunk, further in


def sweep_cases(without=()):
    """a vertex whose weight sum on one side is below SMIN (the assert of compute_balance_ratio in the trivial sweep, of compute_smallest_in / out_edge
    in the smallest-edge sweep) at chosen lanes; every other vertex is a tooth of ratio 1.0"""
    import sweep_cases as SC
    rng = np.random.default_rng(6105); out = []
    for at in SWEEP_AT:
        for r in range(4):
            n_min = at + 3 + int(rng.integers(0, 4))
            if "sweep trivial" not in without:
                t = SC.tooth(2e-6, 3.0) if r % 2 else SC.tooth(3.0, 2e-6)
                out.append(("sweep trivial", "default", dict(SC.assemble({at: t}, rng, lambda k: SC.flat(rng), n_min), rank=None)))
            if "sweep smallest" not in without:
                b = SC.block((3e-6, 4e-6), (5, 5), (5, 5)) if r % 2 else SC.block((5, 5), (5, 5), (3e-6, 4e-6))
                pos = at if r % 2 else at - 3             # the failing vertex is the block's first (its a) or its last (its z)
                if pos < 1: pos = at
                out.append(("sweep smallest", "default", dict(SC.assemble({pos: b}, rng, lambda k: SC.flat(rng), n_min), rank=None)))
    # a vertex that fires `now` (ratio 0.001 < 0.01) IN FRONT of the failing one, in the same chunk of 64: the reference removes its edge first
    for at in (40, 63, 100, 120):
        for r in range(3):
            if "sweep smallest" in without: continue
            b = SC.block((3e-6, 4e-6), (5, 5), (5, 5)) if r % 2 else SC.block((5, 5), (5, 5), (3e-6, 4e-6))
            out.append(("sweep smallest", "default", dict(SC.assemble({at - 12 - r: SC.cand_a((1, 999)), at: b}, rng, lambda k: SC.flat(rng), at + 5), rank=None)))
    return out


def late_cases(without=()):
    """graphs whose cascade goes through and leaves finished source -> sink edges (n teeth: n paths), and then
      "late direct"  a direct source -> sink edge among them: collect_path's empty vertex list (scallop.cc:2783).  It is the OLDEST of the finished
                     edges (every merged edge is newer than every staged one), so the reference meets it first: the n others must not be published
      "late greedy"  a vertex no rule may touch (one in-edge of strand 1, one out-edge of strand 2: mixed) with an under-weight edge from the source:
                     the n paths ARE collected, then greedy_decompose's balance_vertex asserts"""
    import sweep_cases as SC
    rng = np.random.default_rng(6106); out = []
    for n in (1, 3, 12, 30):
        for r in range(4):
            g = SC.assemble({1: SC.flat(rng)}, rng, lambda k: SC.flat(rng), n)
            V = g["V"]
            if "late direct" not in without:
                d = dict(g, edges=[list(e) for e in g["edges"]] + [[0, V - 1, 7.0, 0, {0: 7.0}]], count=None)
                d["rank"] = [int(x) for x in rng.permutation(len(d["edges"]))]
                out.append(("late direct", "default", d))
            if "late greedy" not in without:
                # two more vertices u, t in front of the sink: source -> u (strand 1, under-weight) -> t (strand 2) -> sink
                h = shapes.open_room(dict(g, phasing=[], count=None), V - 1, 2); u = V - 1; t = V; sink = V + 1
                h["edges"] += [[0, u, 0.004, 1, {0: 1.0}], [u, t, 5.0, 2, {0: 1.0}], [t, sink, 5.0, 0, {0: 1.0}]]
                h["rank"] = [int(x) for x in rng.permutation(len(h["edges"]))]
                out.append(("late greedy", "default", shapes.lay_out(h, rng)))
                # the same with the under-weight edge on the way out (source -> t -> u (mixed) -> sink), and with a weightless COUNT instead: the
                # greedy path runs through u and merge_adjacent_equal_edges meets the count
                for kind in ("out", "count"):
                    h = shapes.open_room(dict(g, phasing=[], count=None), V - 1, 2); t = V - 1; u = V; sink = V + 1
                    h["edges"] += [[0, t, 5.0, 0, {0: 1.0}], [t, u, 5.0, 1, {0: 1.0}], [u, sink, 0.004 if kind == "out" else 5.0, 2, {0: 1.0}]]
                    h["count"] = [1] * len(h["edges"])
                    if kind == "count": h["count"][-1] = 0
                    h["rank"] = [int(x) for x in rng.permutation(len(h["edges"]))]
                    out.append(("late greedy " + kind, "default", shapes.lay_out(h, rng)))
    return out


def raw_cases():
    """raw graphs (handed over before the pre-steps of assembler::assemble, phases as exon-coordinate lists) on which a PRE-STEP asserts:
      "raw boundary"  the start (or end) boundaries do not ascend with the vertex index: assert(p >= p2) / assert(p <= p2) of group_start / end_boundaries
      "raw phase"     a phase whose exons are all known but listed backwards: assert(vv[i] < vv[i + 1]) of build_path_from_exon_coordinates
    -> [(label, single-graph PackedGraphs, phases)]"""
    import sweep_cases as SC
    rng = np.random.default_rng(6108); out = []
    for r in range(12):
        n = 3 + r % 4
        g = SC.comb([(5 + j, 5 + j) for j in range(n)], rng)
        a, b = (1, 2) if r % 2 == 0 else (n - 1, n)           # the first two teeth (start boundaries) or the last two (end boundaries)
        h = dict(g, lpos=list(g["lpos"]), rpos=list(g["rpos"]))
        h["lpos"][a], h["lpos"][b] = g["lpos"][b], g["lpos"][a]; h["rpos"][a], h["rpos"][b] = g["rpos"][b], g["rpos"][a]
        out.append(("raw boundary", shapes.pack([dict(h, phasing=[])]), []))
        x, y = 1 + r % (n - 1), 2 + r % (n - 1)
        out.append(("raw phase", shapes.pack([dict(g, phasing=[])]), [([g["lpos"][y], g["rpos"][y], g["lpos"][x], g["rpos"][x]], 2 + r % 3)]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# witnesses: graphs that end with status 0 and need what a predecessor in the same wave may have left behind
# ---------------------------------------------------------------------------------------------------------------------------------------
WITNESS_KINDS = ("a", "b", "c", "d", "e", "f")


def witnesses(repeat=4):
    """[(kind, graph)], to be run under the `wide` parameters:
      a  grows past its own V (a router's decomposition adds vertices)          d  edges with several samples
      b  takes edge slots beyond its own E and reuses freed ones                e  much smaller than any failing graph (4 .. 6 vertices)
      c  has phasing lists                                                      f  two hubs in one sweep: the pairs of the first are parked while the second is routed
    what each really does is asserted from the oracle's statistics in tests/test_assert_exits_cpu.py"""
    import sweep_cases as SC
    rng = np.random.default_rng(6107); out = []
    for r in range(repeat):
        kin, kout = ((2, 2), (3, 3), (2, 3), (3, 4))[r % 4]
        out.append(("a", hub(rng, kin, kout)))
        kin, kout = ((3, 3), (2, 3), (3, 4), (4, 4))[r % 4]
        full = [(i, j, 2 + (i + j) % 3) for i in range(kin) for j in range(kout)]
        out.append(("b", hub(rng, kin, kout, routes=full)))
        out.append(("c", dict(shapes.lay_out(shapes.star(rng, 3 + r, r % 2 == 0, weights="tied", phasing=True, stem=True), rng), rank=None)))
        out.append(("d", dict(shapes.lay_out(shapes.star(rng, 2 + r, r % 2 == 1, weights="random", samples=4), rng), rank=None)))
        out.append(("e", dict(SC.comb([(5 + r, 5 + r)] * (2 + r % 3), rng), rank=None)))
        g = shapes.router(rng, 5 + r, 6, weights="tied", guard=True)
        g = shapes.router(rng, 4, 4 + r, base=g, weights="tied", guard=True)
        out.append(("f", dict(shapes.lay_out(g, rng), rank=None)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# everything, run once
# ---------------------------------------------------------------------------------------------------------------------------------------
GENERATORS = dict(star=star_cases, extreme=extreme_star_cases, late_count=late_count_cases, router=router_cases, router_param=router_param_cases, sweep=sweep_cases, late=late_cases)


def all_cases(without=()):
    """[(label, parameter set, graph)] of every generator; without: labels left out"""
    out = []
    for name, fn in GENERATORS.items(): out += fn(without=without)
    return out


def site_batches(without=()):
    """the failing graphs, one batch per parameter set -> {parameter set: (labels, PackedGraphs, graphs, parameters)}"""
    key = ("site", tuple(sorted(without)))
    if key not in _CACHE:
        by = {}
        for label, ps, g in all_cases(without): by.setdefault(ps, []).append((label, g))
        _CACHE[key] = {ps: ([l for l, _ in v], pack([g for _, g in v]), [g for _, g in v], params(**PARAM_SETS[ps])) for ps, v in by.items()}
    return _CACHE[key]


def kernel_fail_lines(header="decomp_device.h"):
    """{line: status expression} of every fail(...) of the engine header that the emulation COMPILES and whose status is not a plain capacity word
    (ALD_ST_CAPACITY / ALD_ST_POOL_FULL): the ALD_ST_INVARIANT exits and the ones that pass a status on (fail(code), fail(inv[q]), fail(ctx[SW_FAIL])).
    Which lines are compiled is the preprocessor's answer, not a list of macro names kept here: the header goes through `g++ -E` with the
    emulation's flags for a class of each kind, and fail(st) expands to fail_((st), __LINE__), so the line numbers are in the output"""
    key = ("fail_lines", header)
    if key not in _CACHE:
        import subprocess
        path = os.path.join(shapes.CSRC, header); src = open(path).read().split("\n"); compiled = set()
        for cid in (0, 2, 10, 13):
            r = subprocess.run(["g++", "-E", "-std=c++17", "-DALD_EMU", "-DALD_RAW_VARIANT", "-DALD_CLASS_ID=%d" % cid, "-x", "c++", path], capture_output=True, text=True, check=True)
            compiled |= {int(m.group(1)) for m in re.finditer(r"\bfail_\s*\(\s*\(.*?\)\s*,\s*(\d+)\s*\)", r.stdout)}
        out = {}
        for no in sorted(compiled):
            for m in re.finditer(r"\bfail\(([^;]*?)\);", src[no - 1]):
                if m.group(1).strip() not in ("ALD_ST_CAPACITY", "ALD_ST_POOL_FULL"): out[no] = m.group(1).strip()
        assert len(out) >= 30, "the fail() exits of %s were not found" % header
        _CACHE[key] = out
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------------
# the sites a crude random probe reaches (3 000 seeded random graphs per mode): they must be reached here and may not be declared unreachable
PROBE_SITES = ("Scallop::merge_adjacent_equal_edges: ei1.count > 0 && ei2.count > 0", "Scallop::balance_vertex: in-edge weight", "Scallop::balance_vertex: out-edge weight",
               "Router::classify: !gr.mixed_strand_vertex(root)", "UGraph::add_edge: s >= 0 && s < num_vertices()", "UGraph::add_edge: t >= 0 && t < num_vertices()",
               "Router::classify_plain_vertex: ug.degree(i) >= 1", "Scallop::collect_path: !v.empty() && v[0] > 0 && v.back() < n")
DEGREE_SITE = "Scallop::decompose_vertex_replace: gr.degree(root) == 0"
NAN_SITE = "Scallop::decompose_vertex_replace: w >= cfg.min_guaranteed_edge_weight - SMIN"
MERGE_EQUAL_SITE = "Scallop::merge_adjacent_equal_edges: fabs(wx0 - wy0) <= SMIN"
STAR_SITES = PROBE_SITES[:3] + (DEGREE_SITE, NAN_SITE, MERGE_EQUAL_SITE)                        # met inside decompose_trivial_vertex: counted per fan bucket and direction
ROUTER_SITES = PROBE_SITES[3:7] + ("Scallop::decompose_vertex_extend: ei1.count > 0 && ei2.count > 0", "Scallop::decompose_vertex_extend: ei.count > 0")
ROUTER_FORMS = ("2+2", "small below LP", "small at and above LP", "large")

# kernel exits no graph reaches.  Key: a piece of the source line (every fail() line of decomp_device.h that contains it is meant); value: why.
# Every entry is an argument why no input reaches the line; an entry that says `not covered` is refused by the test.
UNREACHED = {
    "(int)cur != e": "cannot happen on a consistent state: the edge being unlinked or re-sorted is in the list of the endpoint its own link word names, so the walk finds it before the list ends",
    "if(ALD_UNLIKELY(!seen))": "cannot happen on a consistent state: the insertion walk starts at an edge that is a member of the list it walks, so it is seen before the list ends",
    "!(w >= HC.p_min_w - kSMIN)": "cannot happen: split_edge is only called by the greedy phase, with the bottleneck weight of a source-sink path.  compute_maximum_path takes min(edge weight, what the path carried so far) with `xw < ts ? xw : ts`, which skips a NaN, so the bottleneck is the weight of a real edge of the path or the DBL_MAX the source starts with; every edge of such a path has an inner endpoint with edges on both sides, and both balance passes leave each edge of such a vertex at min_w or more (the clamp, then a non-negative fix-up)",
    "if(ALD_UNLIKELY(!(ww >= mw - kSMIN)))": "cannot happen: the general merge is only called by the greedy phase with that same bottleneck weight -- the weight of an edge both balance passes left at min_w or more, or DBL_MAX (see split_edge)",
    "fabs(wx0 - wy0) <= kSMIN": "cannot happen: the general merge is only called by the greedy phase, whose cut weight ww is finite -- compute_maximum_path starts the source at DBL_MAX and takes minima, so ww <= DBL_MAX even over infinite edges.  Each of the two pieces is then a fresh piece of weight exactly ww, an edge within SMIN of ww, or the running edge 0.5 * a + 0.5 * b of two such: all lie in [ww - SMIN, ww + SMIN] on the side of the path's minimum, ww itself, so they differ by SMIN at most.  (In a STAR the pair weight can be infinite: those forms report the class on their failing exits, see the overflow stars)",
    "not a trivial vertex": "cannot happen: every caller has tested that one side of the vertex has exactly one edge, and a fan cannot hold more edges than the class has slots",
    "mdeg[i] == 0": "cannot happen: classify has checked that every node of the bipartite graph has an edge, and thread() turns every edge of that graph into a pair, so every edge of the root is in a pair",
    "evx[u1] < 0": "cannot happen: a pair whose second edge has one pair only and whose first has one as well got a vertex in the loop above; if the first has two or more it got one in the loop before",
    "H.vx[root].in_deg != 0 ||": "cannot happen on a consistent state: every edge of the root is in a pair (see mdeg) and every pair moves its edges off the root",
    "assert(ve.size() >= 1)": "cannot happen on a consistent state: a vertex leaves the nonzero set in the same step that takes its last edge",
    "assert(e2u.find(e2) != end)": "cannot happen on a consistent state: a phasing list is a path, so the edge behind an in-edge of the root leaves the root, and the list edits keep that",
    "if(ALD_UNLIKELY(s < 0 || t < 0))": "cannot happen on a consistent state: both edges of a route are live edges of the root (the two tests in front of it), so both are among its gathered edges",
    "if(ALD_UNLIKELY(b1 || b2))": "cannot happen: every node has an edge (checked two lines above) and every edge joins the two sides, so a side that lies in one component pulls the whole other side into it -- one component, not several",
    "if(ALD_UNLIKELY(b < 1))": "cannot happen: every node has an edge, so no component is a single node and at least one has two nodes",
    "!(vw[t] >= vw[x])": "cannot happen for weights that compare (no NaN): x has the smallest weight among the nodes of degree two or more, and a neighbour of degree one with a smaller weight would have been threaded as a leaf first",
    "if(ALD_UNLIKELY(live != 0))": "cannot happen for weights that compare (no NaN): the loop only stops when no node has two edges, and an edge between two nodes of degree one is a leaf for the lighter of them",
    "if(ALD_UNLIKELY(bad)) { fail(ALD_ST_INVARIANT + ALD_INV_ROUTER)": "cannot happen for weights that compare (no NaN) -- the 2 + 2 form of the same turn assert: the node taken has the smallest weight among those with two edges, and a lighter leaf next to it would have gone first (no NaN)",
    "qt != n": "cannot happen: staging only accepts edges from a lower to a higher vertex index and no rule adds an edge against that order, so the graph has no cycle and the sort reaches every vertex",
    "if(ALD_UNLIKELY(ee < 0))": "cannot happen on a consistent state: the general merge returns -1 without a status only for edges that are dead or do not meet, and consecutive edges of the path just computed are live and meet",
    "guard <= 0) fail(": "cannot happen: the guard counts the turns of the cascade, each of which removes a vertex or an edge; it is a bound against an endless loop, not an assert of the reference",
}


def unreached_lines(header="decomp_device.h"):
    """{line: reason} for the fail() lines of the header that UNREACHED names; raises when a key matches no line (a stale entry)"""
    lines = kernel_fail_lines(header); src = open(os.path.join(shapes.CSRC, header)).read().split("\n"); out = {}
    for key, reason in UNREACHED.items():
        hit = [ln for ln in lines if key in src[ln - 1]]
        assert hit, "UNREACHED names no line of %s: %r" % (header, key)
        for ln in hit: out[ln] = reason
    return out


def star_form_lines(src):
    """(first, last) line of the star forms in decomp_device.h: from STAR_MAX to the decomposition behind the router"""
    lo = next(i for i, l in enumerate(src, 1) if re.search(r"enum\s*\{\s*STAR_MAX", l))
    hi = next(i for i, l in enumerate(src, 1) if "scallop::decompose_vertex_extend (scallop.cc:1675-1986); pe2w" in l)
    assert lo < hi
    return lo, hi


def oracle_of(ps, without=()):
    key = ("oracle", ps, tuple(sorted(without)))
    if key not in _CACHE:
        labels, pg, graphs, prm = site_batches(without)[ps]
        _CACHE[key] = common.oracle_assert_sites(pg, threads=DR.THREADS, params=prm)
    return _CACHE[key]


def raw_results():
    """the raw cases through the oracle's pre-steps and the raw build of the emulation -> (oracle status per item, site names, emulation status, lines)"""
    if "raw" not in _CACHE:
        import ctypes as C
        O = common.oracle_lib()
        O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]; O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
        O.ora_pre_assemble_site.restype = C.c_char_p
        rc = []; sites = []; items = []
        for label, pg, ph in raw_cases():
            rc.append(int(A.pre_assemble(pg, ph, 10000, _lib=O, _prefix="ora")[3])); sites.append(O.ora_pre_assemble_site().decode()); items.append((pg, ph, 10000))
        r, it, cl, tr, ln = common.emu_run_raw(items, full="lines")
        _CACHE["raw"] = (rc, sites, r.status.copy(), ln)
    return _CACHE["raw"]


def router_form(nin, nout, routes):
    n = nin + nout
    if n == 4: return "2+2"
    if K["router_small"](nin, nout, routes): return "small below LP" if n < K["LP"] else "small at and above LP"
    return "large"


class Census:
    def __init__(self):
        self.sites = {}; self.stars = {}; self.routers = {}; self.lines = {}; self.site_lines = {}

    def add(self, site, line, has_routes):
        name, v, din, dout = site
        self.sites[name] = self.sites.get(name, 0) + 1
        self.site_lines.setdefault(name, set()).add(int(line))
        if name in STAR_SITES and v >= 0 and (din == 1 or dout == 1):
            key = (name, shapes.fan_bucket(dout if din == 1 else din, K), "out" if din == 1 else "in")
            self.stars[key] = self.stars.get(key, 0) + 1
        if name in ROUTER_SITES and din >= 2 and dout >= 2:
            key = (name, router_form(din, dout, has_routes))
            self.routers[key] = self.routers.get(key, 0) + 1

    def site_lines_of(self, names):
        return sorted(set(ln for n in names for ln in self.site_lines.get(n, ()) if ln))

    def required(self):
        out = {}
        for name in sorted(set(self.sites) | set(PROBE_SITES)): out["site " + name] = self.sites.get(name, 0)
        for name in STAR_SITES:
            for fb in shapes.fan_buckets(K):
                for d in ("in", "out"):
                    if star_exemption(name, fb, d) is None: out["star %s | fan %s %s" % (name.split(": ")[1][:28], fb, d)] = self.stars.get((name, fb, d), 0)
        for name in ROUTER_SITES:
            for form in ROUTER_FORMS:
                if router_exemption(name, form) is None: out["router %s | %s" % (name.split(": ")[1][:28], form)] = self.routers.get((name, form), 0)
        return out

    def table(self):
        rows = ["%-78s %5d" % kv for kv in self.required().items()]
        lines = kernel_fail_lines(); listed = unreached_lines()
        rows += ["line %-5d %-44s %5s" % (ln, lines[ln][:44], "unreached (listed)" if ln in listed else self.lines.get(ln, 0)) for ln in sorted(lines)]
        return "\n".join(rows)


def star_exemption(site, bucket, direction):
    """None, or why a (site, fan bucket, direction) line of the census cannot hold an event"""
    if bucket == "1" and direction == "in": return "a vertex with one edge on each side is taken as a fan that goes out"
    if site == DEGREE_SITE and bucket == "1": return "with one fan edge the centre starts as exactly that pair weight and the one merge uses it up"
    if site == NAN_SITE and direction == "in": return "a fan that comes in takes min(fan, centre) with the fan first, so a NaN fan weight loses to the centre's: no pair weight is NaN"
    if site == NAN_SITE and bucket == "1": return "the one fan edge would have to be the weightless one, and the sweep's own weight sum assert comes first"
    return None


def router_exemption(site, form):
    if form == "small at and above LP":
        LP = K["LP"]
        if not any(K["router_small"](a, n - a, False) for n in range(LP, LP + 8) for a in range(2, n - 1)):
            return "this build has no such form: the arena limit of the small form (5 n + 3 n <= ARENA_I, 4 n <= ARENA_D) lies below LP"
        if site.startswith("Scallop::decompose_vertex_extend"):
            return "both count exits need a pair whose two edges have two pairs each, which only routes give; with routes the small form ends below LP (bound + n <= LP)"
    return None


def census(without=()):
    """the census of the site batches: sites, degrees and traces from the oracle, lines from the list build of the emulation -- run with the op trace
    and without it (the collect phase publishes a whole round of finished edges at once when nothing is traced) -- plus the raw cases"""
    key = ("census", tuple(sorted(without)))
    if key not in _CACHE:
        c = Census()
        for ps, (labels, pg, graphs, prm) in site_batches(without).items():
            want, traces, sites = oracle_of(ps, without)
            ln = common.emu_run_full(pg, params=prm)[4]
            ln0 = common.emu_run_full(pg, params=prm, cap=0)[4]
            for g in range(pg.n):
                if sites[g] is not None: c.add(sites[g], ln[g], int(pg.g_np[g]) > 0)
                for x in {int(ln[g]), int(ln0[g])}: c.lines[x] = c.lines.get(x, 0) + 1
        if not without:
            rc, sites, status, ln = raw_results()
            for s, x in zip(sites, ln):
                c.sites[s] = c.sites.get(s, 0) + 1; c.lines[int(x)] = c.lines.get(int(x), 0) + 1
        _CACHE[key] = c
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the graph behind a failed one
# ---------------------------------------------------------------------------------------------------------------------------------------
SUCCESSOR_GROUPS = {"star count": ("star count", "star centre count", "star two counts", "late count"),
                    "star weight": ("star weight", "star centre weight", "star count and weight"),
                    "router strand": ("router strand",), "router classify": ("router no partner", "router bare node"),
                    "router decomposition": ("router count", "router empty pair"),
                    "late exit": ("late direct", "late greedy", "late greedy out", "late greedy count"), "sweep exit": ("sweep trivial", "sweep smallest")}
SUCCESSOR_CLASS = 2                       # the first class pick_class may choose: every graph of the batch fits it, so ONE work list holds them all, in the order given
PER_PAIR = 12


def successor_batch(per_pair=PER_PAIR):
    """failed graph, witness, failed graph, witness ... under the `wide` parameters (the witnesses of kind f need them, and no failing graph of the
    default set ends differently under them): per exit group per_pair x 6 failing graphs drawn across the group's families, the witness kinds in turn"""
    key = ("successor", per_pair)
    if key not in _CACHE:
        cases = [(l, g) for l, ps, g in all_cases() if ps in ("default", "wide")]
        wit = {k: [g for kk, g in witnesses(repeat=6) if kk == k] for k in WITNESS_KINDS}
        graphs = []; labels = []; kinds = []
        for group, fam in SUCCESSOR_GROUPS.items():
            pool = [(l, g) for l, g in cases if l in fam]
            assert pool, group
            step = max(1, len(pool) // (per_pair * len(WITNESS_KINDS)))
            for i in range(per_pair * len(WITNESS_KINDS)):
                l, g = pool[(i * step) % len(pool)]; k = WITNESS_KINDS[i % len(WITNESS_KINDS)]
                graphs += [g, wit[k][(i // len(WITNESS_KINDS)) % len(wit[k])]]; labels += [l, "witness " + k]; kinds += [group, k]
        pg = pack(graphs); prm = params(**PARAM_SETS["wide"])
        want, traces, sites = common.oracle_assert_sites(pg, threads=DR.THREADS, params=prm)
        _CACHE[key] = dict(pg=pg, params=prm, graphs=graphs, labels=labels, kinds=kinds, want=want, traces=traces, sites=sites)
    return _CACHE[key]


def successor_pairs(o, classes):
    """(exit group, witness kind) -> how often a graph that FAILED is directly followed by a witness in the work list of its class (the lists hold
    the graphs of a class in batch order)"""
    out = {}
    for c in sorted(set(int(x) for x in classes)):
        seq = [g for g in range(len(classes)) if int(classes[g]) == c]
        for x, y in zip(seq, seq[1:]):
            if o["kinds"][x] in SUCCESSOR_GROUPS and o["want"].status[x] != 0 and o["kinds"][y] in WITNESS_KINDS and o["want"].status[y] == 0:
                k = (o["kinds"][x], o["kinds"][y]); out[k] = out.get(k, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the device side (tests/test_assert_exits_gpu.py, tools/assert_exits_parity.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
TRACE_CAP = 256                           # the longest op trace is that of a 70-edge `remainder` star that ends well: 1 + 70 + 70 events (asserted where it is used)
SLAB_CLASS_GRAPHS = 80                    # graphs per batch in the classes whose state lives in a slab of 13 MB and more per wave (what the class matrix runs there)


def site_mismatches_on_device(first, twin, cls=None):
    """every site batch with the first class forced -> (graphs run, mismatches); cls: the class the small graphs must end in (None: not checked).
    The classes whose state lives in the slab take an even-stride sample of SLAB_CLASS_GRAPHS graphs per parameter set"""
    tot = 0; bad = []
    for ps, (labels, pg, graphs, prm) in site_batches().items():
        want, traces, sites = oracle_of(ps)
        assert max(len(t) for t in traces) < TRACE_CAP
        idx = np.arange(pg.n)
        if cls is not None and cls >= 10: idx = idx[::max(1, -(-pg.n // SLAB_CLASS_GRAPHS))]
        r = DR.run(pg.select(idx) if len(idx) < pg.n else pg, prm, first=first, twin=twin, trace_cap=TRACE_CAP)
        tag = "%s, first class %d, twin %s" % (ps, first, twin)
        if cls is not None and cls not in r.classes: bad.append((tag, "classes", r.classes))
        bad += DR.oracle_mismatches(tag, r, common.select_results(want, idx), None, traces, traced=idx,
                                    want_classes=None if cls is None else set(range(cls, DR.N_CLASSES)))
        tot += len(idx)
    return tot, bad


def raw_star_and_late_items(stride=4):
    """the star and late-exit cases of the default parameter set in RAW form (no phases; the load phase of the raw build folds the boundary edges at
    the source and the sink first) -> (batch for add_packed_raw, the oracle's staged graphs, labels, cases the raw entry point does not take).
    Every fan size of STAR_FANS, every stride-th case (the 70-edge fan has 73 vertices and takes class 1 or 2 whatever is forced).  A case is left
    out only when the ORACLE's pre-steps assert on it; the caller asserts how many."""
    if "rawform" not in _CACHE:
        import ctypes as C
        O = common.oracle_lib()
        O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]; O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
        cases = [(l, g) for l, ps, g in star_cases() if ps == "default"][::stride] + [(l, g) for l, ps, g in late_cases()] + [(l, g) for l, ps, g in late_count_cases()][::2]
        raws = []; staged = []; labels = []; dropped = 0
        for l, g in cases:
            one = pack([g])
            want, _, _, rc = A.pre_assemble(one, [], 10000, _lib=O, _prefix="ora")
            if rc != 0: dropped += 1; continue
            raws.append(one); staged.append(want); labels.append(l)
        _CACHE["rawform"] = (PackedGraphs.concat(raws), PackedGraphs.concat(staged), labels, dropped)
    return _CACHE["rawform"]


def order_batch(copies):
    """the interleaved batch of the CPU tier, `copies` times over (each copy the same graphs: the order is what varies)"""
    o = successor_batch(); n = o["pg"].n
    idx = np.concatenate([np.arange(n)] * copies)
    return o, idx


# two more exit groups, each in an interleaved batch of its own (a parameter / an environment word holds for a whole batch):
#   "grown past max_num_exons"  hubs of 37 vertices under max_num_exons = 38: the router's decomposition adds vertices, the cascade stops with
#                               ALD_ST_SKIPPED_LARGE in the middle of the run (what is finished by then is published, as the reference does)
#   "capacity climb"            hubs whose routes make 400 new edges, started one class too low (ALD_DEBUG_UNDERCLASS=1): ALD_ST_CAPACITY where the
#                               decomposition behind the router asks for slots, pairs parked, then the same graph again one class up
GROWN_MAX_EXONS = 38                      # the hubs have 37 vertices and grow to 39


def extra_successor_batch(which, per_pair=16):
    key = ("successor2", which, per_pair)
    if key not in _CACHE:
        rng = np.random.default_rng(6111 if which == "grown" else 6112)
        wit = {k: [g for kk, g in witnesses(repeat=6) if kk == k] for k in WITNESS_KINDS}
        group = "grown past max_num_exons" if which == "grown" else "capacity climb"
        graphs = []; labels = []; kinds = []
        for i in range(per_pair * len(WITNESS_KINDS)):
            if which == "grown": g = hub(rng, 17, 17, w=float(3 + i % 5))
            else: g = hub(rng, 20, 20, routes=[(a, b, 2 + (a + b) % 3) for a in range(20) for b in range(20)], w=float(3 + i % 5))
            k = WITNESS_KINDS[i % len(WITNESS_KINDS)]
            graphs += [g, wit[k][(i // len(WITNESS_KINDS)) % len(wit[k])]]; labels += [group, "witness " + k]; kinds += [group, k]
        pg = pack(graphs); prm = params(r0=0.0, max_exons=GROWN_MAX_EXONS) if which == "grown" else params(**PARAM_SETS["wide"])
        want, st, _, traces = common.oracle_run(pg, threads=DR.THREADS, trace=True, params=prm)
        _CACHE[key] = dict(pg=pg, params=prm, graphs=graphs, labels=labels, kinds=kinds, want=want, traces=traces, stats=st, group=group)
    return _CACHE[key]
