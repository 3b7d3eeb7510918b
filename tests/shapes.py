"""Hub-shaped splice graphs for the parity tests (tests/test_hub_shapes_cpu.py, tests/test_hub_shapes_gpu.py).

The decomposition kernel chooses its code path by the DEGREE of the vertex at hand (decomp_device.h: star_fixed / star_reg / the sequential
star, router_22 / router_small / router_large), and A.synth's uniform random DAGs hardly ever reach the degrees where one form hands over to
the next.  The generators here build those degrees on purpose: single hubs with a fan of exactly k edges in either direction, k_in x k_out
hubs the router has to split, each alone, with a random tail, or spliced into a synth graph at a chosen vertex index.  Everything is seeded.

The thresholds the tests name are read from the kernel headers (kernel_constants), the census of what a batch exercised is taken in the
oracle (census_of / Census), and hub_batch() is the batch both tiers run."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

import aletsch_amd as A
from aletsch_amd.packed import PackedGraphs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aletsch_amd", "csrc")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the form thresholds, read from the kernel headers
# ---------------------------------------------------------------------------------------------------------------------------------------
def _c_condition(expr: str):
    """a C integer condition over named values -> a Python function of those names (&&, ||, !defined(...) only)"""
    py = re.sub(r"!\s*defined\s*\(\s*\w+\s*\)", "True", expr).replace("&&", " and ").replace("||", " or ")
    assert re.fullmatch(r"[\w\s()<>=+*\-]+", py), expr
    code = compile(py, "<kernel header>", "eval")
    return lambda **names: bool(eval(code, {"__builtins__": {}}, names))


def kernel_constants():
    """STAR_MAX, LP, ARENA_I, ARENA_D, ALD_STARFIX_MAX per size class and the router's `small` predicate as decomp_device.h states them;
    raises when one of them cannot be found (a test that names a threshold must not carry a copy that can drift)"""
    src = open(os.path.join(CSRC, "decomp_device.h")).read()
    common = open(os.path.join(CSRC, "decomp_common.h")).read()
    out = {}
    m = re.search(r"enum\s*\{\s*STAR_MAX\s*=\s*(\d+)\s*\}", src)
    assert m, "STAR_MAX not found in decomp_device.h"
    out["STAR_MAX"] = int(m.group(1))
    m = re.search(r"enum\s*\{\s*LP\s*=\s*(\d+)\s*,\s*ARENA_I\s*=\s*(\d+)\s*,\s*ARENA_D\s*=\s*(\d+)", src)
    assert m, "LP / ARENA_I / ARENA_D not found in decomp_device.h"
    out["LP"], out["ARENA_I"], out["ARENA_D"] = (int(x) for x in m.groups())
    m = re.search(r"#ifndef ALD_STARFIX_MAX\s*\n(?:\s*//[^\n]*\n)*\s*#if\s+([^\n]+)\n\s*#define ALD_STARFIX_MAX (\d+)\s*\n\s*#else\s*\n\s*#define ALD_STARFIX_MAX (\d+)", src)
    assert m, "the per-class ALD_STARFIX_MAX not found in decomp_device.h"
    roomy = _c_condition(m.group(1))
    m2 = re.search(r"#define ALD_NUM_CLASSES\s+(\d+)", common)
    assert m2, "ALD_NUM_CLASSES not found in decomp_common.h"
    out["NUM_CLASSES"] = int(m2.group(1))
    out["STARFIX_MAX"] = [int(m.group(2)) if roomy(ALD_CLASS_ID=c) else int(m.group(3)) for c in range(out["NUM_CLASSES"])]
    m = re.search(r"ALD_INL bool router_run\(.*?const bool small\s*=\s*([^;]+);", src, re.S)
    assert m, "router_run's `small` test not found in decomp_device.h"
    small = _c_condition(m.group(1))
    out["router_small"] = lambda nin, nout, routes: small(n=nin + nout, route_bound=nin * nout if routes else 0, LP=out["LP"], ARENA_I=out["ARENA_I"], ARENA_D=out["ARENA_D"])
    feat = open(os.path.join(CSRC, "trst_features_dev.h")).read()
    m = re.search(r"enum\s*\{\s*FT_LDS_WORDS\s*=\s*(\d+)\s*\}", feat)
    assert m, "FT_LDS_WORDS not found in trst_features_dev.h"
    out["FT_LDS_WORDS"] = int(m.group(1))
    m = re.search(r"static inline int class_twin\(int c\)\s*\{\s*return c == (\d+) \? (\d+) : c == (\d+) \? (\d+)", common)
    assert m, "class_twin not found in decomp_common.h"
    out["TWINS"] = {int(m.group(1)): int(m.group(2)), int(m.group(3)): int(m.group(4))}
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# graph dicts: unpack a synth graph, open room in it, mirror it, pack a list of them (with edge counts and creation ranks)
# ---------------------------------------------------------------------------------------------------------------------------------------
def unpack(pg: PackedGraphs, g: int) -> dict:
    """graph g of a packed batch as a dict of the form PackedGraphs.from_graphs takes; edges are LISTS [s, t, w, strand, {sid: abd}]"""
    o = pg.graph_slices()
    V, E, NP = int(pg.g_nv[g]), int(pg.g_ne[g]), int(pg.g_np[g])
    vo = pg.vertex_offset[o["vo"][g]:o["vo"][g] + V + 1]; eo = pg.edge_sample_offset[o["eo"][g]:o["eo"][g] + E + 1]
    e0, s0, v0 = int(o["e"][g]), int(o["s"][g]), int(o["v"][g])
    edges = []
    for s in range(V):
        for k in range(int(vo[s]), int(vo[s + 1])):
            sp = {int(pg.sample_id[s0 + j]): float(pg.sample_abd[s0 + j]) for j in range(int(eo[k]), int(eo[k + 1]))}
            edges.append([s, int(pg.edge_target[e0 + k]), float(pg.edge_weight[e0 + k]), int(pg.edge_strand[e0 + k]), sp])
    po = pg.phasing_offset[o["po"][g]:o["po"][g] + NP + 1]
    ph = [([int(x) for x in pg.phasing_vertex[o["pv"][g] + int(po[p]):o["pv"][g] + int(po[p + 1])]], int(pg.phasing_count[o["p"][g] + p])) for p in range(NP)]
    return dict(V=V, edges=edges, vw=[float(x) for x in pg.vertex_weight[v0:v0 + V]], phasing=ph, strand=chr(int(pg.graph_strand[g])))


def empty_graph() -> dict:
    return dict(V=2, edges=[], vw=[0.0, 0.0], phasing=[], strand=".")


def open_room(g: dict, at: int, m: int) -> dict:
    """m new vertices at index `at` (1 <= at <= V - 1): the vertices from `at` on move up by m"""
    assert 1 <= at <= g["V"] - 1
    mv = lambda x: x + m if x >= at else x
    return dict(V=g["V"] + m, edges=[[mv(e[0]), mv(e[1])] + list(e[2:]) for e in g["edges"]], vw=g["vw"][:at] + [0.0] * m + g["vw"][at:],
                phasing=[([mv(x) for x in v], c) for v, c in g["phasing"]], strand=g["strand"],
                count=None if g.get("count") is None else list(g["count"]))


def mirror(g: dict) -> dict:
    """the same graph read from the sink: vertex i becomes V - 1 - i and every edge turns round (an out-fan becomes an in-fan)"""
    V = g["V"]; f = lambda x: V - 1 - x
    return dict(V=V, edges=[[f(e[1]), f(e[0])] + list(e[2:]) for e in g["edges"]], vw=g["vw"][::-1], phasing=[(sorted(f(x) for x in v), c) for v, c in g["phasing"]],
                strand={"+": "-", "-": "+"}.get(g["strand"], g["strand"]), count=None if g.get("count") is None else list(g["count"]))


def lay_out(g: dict, rng, touch: float = 0.2) -> dict:
    """exon coordinates for every vertex, ascending; some neighbours touch (their exons fuse in a transcript)"""
    V = g["V"]; lpos = [0] * V; rpos = [0] * V; pos = 1000
    for i in range(1, V - 1):
        l = rpos[i - 1] if (i > 1 and rng.random() < touch) else pos
        ln = int(rng.integers(50, 400)); lpos[i] = l; rpos[i] = l + ln; pos = rpos[i] + int(rng.integers(100, 900))
    lpos[0] = rpos[0] = lpos[1] if V > 2 else 0
    lpos[V - 1] = rpos[V - 1] = rpos[V - 2] if V > 2 else 0
    g["lpos"], g["rpos"] = lpos, rpos
    g["vw"] = [0.0] + [float(x) if x > 0 else float(rng.integers(1, 40)) for x in g["vw"][1:-1]] + [0.0]
    return g


def pack(graphs, rng=None, permute_rank=()) -> PackedGraphs:
    """PackedGraphs.from_graphs plus the two columns it does not take: g["count"] (edge_info.count per edge, in the order of g["edges"];
    None: the number of samples) and, for the graphs whose index is in permute_rank, a random creation rank"""
    counts = []; ranks = []; any_count = any(g.get("count") is not None for g in graphs); sorted_graphs = []
    for i, g in enumerate(graphs):
        order = sorted(range(len(g["edges"])), key=lambda k: (g["edges"][k][0], g["edges"][k][1]))
        edges = [tuple(g["edges"][k]) for k in order]
        sorted_graphs.append(dict(g, edges=edges))
        cnt = g.get("count")
        counts.append(np.array([len(e[4]) if len(e) > 4 and e[4] is not None else 1 for e in edges] if cnt is None else [cnt[k] for k in order], np.int32))
        ranks.append(rng.permutation(len(edges)).astype(np.int32) if i in permute_rank else np.arange(len(edges), dtype=np.int32))
    pg = PackedGraphs.from_graphs(sorted_graphs)
    if any_count:
        pg.edge_count = np.concatenate(counts).astype(np.int32)
    if len(permute_rank):
        pg.edge_rank = np.concatenate(ranks).astype(np.int32)
    return pg


def synth_base(seed: int, V: int, epv: int = 3, **kw) -> dict:
    """one A.synth graph of V vertices as a dict: the tail / the surroundings a hub is spliced into"""
    return unpack(A.synth(seed=seed, n_graphs=1, v_min=V, v_max=V, edges_per_vertex=epv, **kw), 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the hubs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _samples(rng, w, ns):
    """a sample set of ns samples; sample 0 supports every edge, so that intersections along a path never go empty"""
    if ns <= 1:
        return {0: float(w)}
    ids = [0] + sorted(int(x) for x in rng.choice(np.arange(1, 8), size=ns - 1, replace=False))
    return {i: float(rng.integers(1, 30)) for i in ids}


def _fan_weights(rng, k, mode):
    """(weight of the centre edge, the k fan weights).  random: floats, the two sides differ; tied: equal integers and a centre that equals
    their sum (every comparison of the decomposition is a tie); remainder: the centre carries more than the fan takes; deficit: less"""
    if mode == "tied":
        t = float(rng.integers(2, 9)); return t * k, [t] * k
    if mode == "tied_int":
        w = [float(x) for x in rng.integers(3, 6, k)]; return float(sum(w)), w
    w = [float(x) for x in (1.0 + 99.0 * rng.random(k))]
    if mode == "remainder":
        return float(sum(w)) * float(1.3 + rng.random()), w
    if mode == "deficit":
        return float(sum(w)) * float(0.3 + 0.5 * rng.random()), w
    return float(sum(w)) * float(0.9 + 0.2 * rng.random()), w


def star(rng, k, out=True, base=None, hub_index=None, same_target=0, to_sink=0, weights="random", samples=1, phasing=False, strand=0,
         zero_count=False, stem=None):
    """A hub with ONE edge on the narrow side and a fan of k edges on the other (out: the fan leaves the hub).

    base: a graph dict the hub is spliced into (None: the hub stands alone between source and sink); hub_index: the vertex index the hub
    gets in the finished graph.  The fan ends in leaves of its own; same_target >= 2 sends that many fan edges into ONE leaf (parallel
    edges inside the fan, relinks that land on the same list), to_sink sends that many straight to the sink.  A leaf continues into the
    base (one or two edges to random later vertices: a short random tail) or, without a base, to the sink.  samples: sample sets of up to
    that many samples per edge; phasing: phasing paths through the hub; zero_count: one fan edge with edge_info.count == 0;
    stem: a vertex between the narrow side and the hub (default: where the phasing paths need one)."""
    if not out:
        # build the mirror image and turn it round: the hub must end up at hub_index
        b = None if base is None else mirror(base)
        leaves = k - max(same_target - 1, 0) - to_sink
        Vfin = (2 if base is None else base["V"]) + 1 + leaves + (1 if (stem or (stem is None and phasing and base is None)) else 0)
        g = star(rng, k, True, b, None if hub_index is None else Vfin - 1 - hub_index, same_target, to_sink, weights, samples, phasing, strand, zero_count, stem)
        assert g["V"] == Vfin
        return mirror(g)
    if stem is None:
        stem = bool(phasing and base is None)
    base = empty_graph() if base is None else base
    leaves = k - max(same_target - 1, 0) - to_sink
    assert leaves >= 0 and k >= 1
    m = 1 + leaves + (1 if stem else 0)
    at = (hub_index - (1 if stem else 0)) if hub_index is not None else int(rng.integers(1, base["V"]))
    g = open_room(base, at, m)
    V = g["V"]; hub = at + (1 if stem else 0); first_leaf = hub + 1; later = list(range(at + m, V - 1)); sink = V - 1
    cw, fw = _fan_weights(rng, k, weights)
    ns = lambda: int(rng.integers(1, samples + 1))
    cnt0 = len(g["edges"]); count = None if g.get("count") is None else list(g["count"])
    new = []
    # the narrow side: from the source, or from an earlier vertex of the base
    src = 0 if (at == 1 or rng.random() < 0.5) else int(rng.integers(1, at))
    if stem:
        new.append([src, at, cw, strand, _samples(rng, cw, ns())]); new.append([at, hub, cw, strand, _samples(rng, cw, ns())])
    else:
        new.append([src, hub, cw, strand, _samples(rng, cw, ns())])
    targets = []
    for j in range(k):
        if j < to_sink:
            targets.append(sink)
        elif same_target >= 2 and j < to_sink + same_target:
            targets.append(first_leaf)
        else:
            targets.append(first_leaf + (j - to_sink - max(same_target - 1, 0)))
    fan_first = len(new)
    for j in range(k):
        new.append([hub, targets[j], fw[j], strand, _samples(rng, fw[j], ns())])
    nxt = {}
    for leaf in range(first_leaf, first_leaf + leaves):
        w_in = sum(fw[j] for j in range(k) if targets[j] == leaf)
        outs = [sink] if not later else sorted(set(int(x) for x in rng.choice(later + [sink], size=int(rng.integers(1, 3)))))
        for t in outs:
            w = w_in / len(outs) * (1.0 if weights.startswith("tied") else float(0.8 + 0.4 * rng.random()))
            new.append([leaf, t, w, strand, _samples(rng, w, ns())])
        nxt[leaf] = outs[0]
    g["edges"] += new
    if zero_count or count is not None:
        count = (count if count is not None else [len(e[4]) for e in g["edges"][:cnt0]]) + [len(e[4]) for e in new]
        if zero_count:
            count[cnt0 + fan_first + int(rng.integers(0, k))] = 0
        g["count"] = count
    if phasing:
        for j in rng.choice(k, size=min(k, int(rng.integers(2, 6))), replace=False):
            t = targets[int(j)]
            if t == sink:
                continue
            if stem and rng.random() < 0.5:
                g["phasing"].append(([at, hub, t], int(rng.integers(2, 9))))
            elif nxt.get(t, sink) != sink:
                g["phasing"].append(([hub, t, nxt[t]], int(rng.integers(2, 9))))
            elif stem:
                g["phasing"].append(([at, hub, t], int(rng.integers(2, 9))))
    return g


def router(rng, kin, kout, base=None, hub_index=None, bypass=True, weights="random", samples=1, phasing=False, strand=0, zero_count=False, guard=True):
    """A k_in x k_out hub the router has to split: feeders a_1 .. a_kin -> hub -> receivers b_1 .. b_kout.

    guard: every feeder has the hub as its only way on and every receiver the hub as its only way in, so that no smallest edge of the hub
    may be removed before the router sees all of it; the bypasses then go round the hub through a vertex of their own, from in front of
    the feeders to behind the receivers.  Without guard the bypasses run feeder -> receiver, and the smallest-edge rule may trim the hub.
    phasing: routes a_i -> hub -> b_j through the hub; zero_count (needs phasing): one hub edge with edge_info.count == 0 that a route covers."""
    base = empty_graph() if base is None else base
    nby = int(rng.integers(1, 4)) if bypass else 0
    m = kin + 1 + kout + (nby if guard else 0)
    at = (hub_index - kin) if hub_index is not None else int(rng.integers(1, base["V"]))
    g = open_room(base, at, m)
    V = g["V"]; hub = at + kin; fa = list(range(at, hub)); rb = list(range(hub + 1, hub + 1 + kout)); later = list(range(at + m, V - 1)); sink = V - 1
    ns = lambda: int(rng.integers(1, samples + 1))
    if weights == "tied":
        t = float(rng.integers(2, 9)); win = [t * kout] * kin; wout = [t * kin] * kout
    else:
        win = [float(x) for x in (5.0 + 95.0 * rng.random(kin))]; wout = [float(x) for x in (5.0 + 95.0 * rng.random(kout))]
    cnt0 = len(g["edges"]); count = None if g.get("count") is None else list(g["count"]); new = []
    for i, a in enumerate(fa):
        if zero_count and i == 0: continue
        src = 0 if (at == 1 or rng.random() < 0.6) else int(rng.integers(1, at))
        new.append([src, a, win[i], strand, _samples(rng, win[i], ns())])
    hub_first = len(new)
    for i, a in enumerate(fa):
        # (the edge with count 0 comes straight from the source: behind a feeder it would meet a merge, and its assert, before any router)
        new.append([0 if (zero_count and i == 0) else a, hub, win[i], strand, _samples(rng, win[i], ns())])
    for j, b in enumerate(rb):
        new.append([hub, b, wout[j], strand, _samples(rng, wout[j], ns())])
    for j, b in enumerate(rb):
        t = sink if (not later or rng.random() < 0.6) else int(rng.choice(later))
        new.append([b, t, wout[j], strand, _samples(rng, wout[j], ns())])
    for q in range(nby):
        w = float(rng.integers(2, 30)) if weights != "tied" else 4.0
        if guard:
            s = 0 if at == 1 else int(rng.integers(0, at)); t = sink if not later else int(rng.choice(later + [sink])); mid = hub + 1 + kout + q
            new.append([s, mid, w, strand, _samples(rng, w, ns())]); new.append([mid, t, w, strand, _samples(rng, w, ns())])
        else:
            new.append([int(rng.choice(fa)), int(rng.choice(rb)), w, strand, _samples(rng, w, ns())])
    g["edges"] += new
    routes = []
    if phasing:
        for _ in range(int(rng.integers(1, 1 + min(6, kin * kout)))):
            routes.append((int(rng.integers(0, kin)), int(rng.integers(0, kout))))
        if zero_count:
            routes.append((0, int(rng.integers(0, kout))))
        for i, j in routes:
            g["phasing"].append(([0 if (zero_count and i == 0) else fa[i], hub, rb[j]], int(rng.integers(2, 9))))
    if zero_count or count is not None:
        count = (count if count is not None else [len(e[4]) for e in g["edges"][:cnt0]]) + [len(e[4]) for e in new]
        if zero_count:
            count[cnt0 + hub_first] = 0                      # the hub's first in-edge (feeder 0), covered by a route
        g["count"] = count
    return g


# ---------------------------------------------------------------------------------------------------------------------------------------
# the census (oracle/oracle_capi.cc: ora_result_census)
# ---------------------------------------------------------------------------------------------------------------------------------------
def census_of(pg: PackedGraphs, threads: int = 1, params=None):
    """run the oracle -> (DecompResult, stats, per-graph list of {key: events}); key = (0, direction, fan, 0, 0, 0) for a trivial
    decomposition (direction 0: the fan leaves the vertex), (1, nin, nout, graph has phasing lists, every counted edge has one sample,
    an edge has count 0) for a router build"""
    import common
    from aletsch_amd.packed import export_via
    O = common.oracle_lib()
    h = C.c_void_p()
    rc = O.ora_run_packed(*pg.c_args(), C.byref(params) if params is not None else None, C.c_int32(threads), C.c_int32(0), C.byref(h))
    assert rc == 0
    r = export_via(O.ora_result_export, h, pg.n)
    st = np.zeros((pg.n, 6), np.int32)
    O.ora_result_stats(h, st.ctypes.data_as(C.POINTER(C.c_int32)))
    out = []
    for g in range(pg.n):
        n = C.c_int32()
        O.ora_result_census(h, C.c_int32(g), C.byref(n), None, C.c_int32(0))
        rows = np.zeros((max(n.value, 1), 7), np.int32)
        O.ora_result_census(h, C.c_int32(g), C.byref(n), rows.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(n.value))
        out.append({tuple(int(x) for x in rows[i, :6]): int(rows[i, 6]) for i in range(n.value)})
    O.ora_result_free(h)
    return r, st, out


def fan_buckets(K: dict):
    """the fan-size buckets, named by their bounds: 1, 2, 3, 4, 5-8, 9..STAR_MAX-1, STAR_MAX, STAR_MAX+1, up to the wave - 1, the wave (64 lanes), wave + 1, beyond"""
    S = K["STAR_MAX"]; W = 64
    assert 9 < S < W - 2
    return ("1", "2", "3", "4", "5-8", "9-%d" % (S - 1), str(S), str(S + 1), "%d-%d" % (S + 2, W - 1), str(W), str(W + 1), ">%d" % (W + 1))


def fan_bucket(fan: int, K: dict) -> str:
    S = K["STAR_MAX"]; W = 64; names = fan_buckets(K)
    bounds = (1, 2, 3, 4, 8, S - 1, S, S + 1, W - 1, W, W + 1)
    for b, name in zip(bounds, names):
        if fan <= b: return name
    return names[-1]


def class_group(cls: int, nv: int, K: dict) -> str:
    """0-1 | 2-9 | twins | 10,13: the groups ALD_STARFIX_MAX distinguishes (a graph of a class that has a twin counts as twin-sized: the twin
    tests run it on both).  The catch-all class and the class beyond it are a group of their own: they share ALD_STARFIX_MAX with classes
    0 / 1 and nothing else (hot state in the slab, kept sweep records, the merged list walks)."""
    if cls in K["TWINS"] or cls in K["TWINS"].values(): return "twins"
    if cls >= 10: return "10,13"
    return "0-1" if cls <= 1 else "2-9"


def router_buckets(key, K: dict):
    """the buckets a router build (census key) belongs to"""
    _, nin, nout, routes, single, zero = key; n = nin + nout; LP = K["LP"]; out = []
    small = K["router_small"](nin, nout, routes)
    if nin == 2 and nout == 2 and not routes and single and not zero: out.append("2+2 plain")
    if nin == 2 and nout == 2 and not (not routes and single): out.append("2+2 routes or samples")
    if not routes:
        for x in (LP - 1, LP, LP + 1):
            if n == x: out.append("n=%d no routes" % x)
        if small and not single: out.append("small, several samples")
        if small and single and n > 4: out.append("small, table")
        if small and not K["router_small"](nin + 1, nout, 0) or small and not K["router_small"](nin, nout + 1, 0): out.append("largest small, no routes")
        if not small and (K["router_small"](nin - 1, nout, 0) or K["router_small"](nin, nout - 1, 0)): out.append("smallest large, no routes")
    else:
        if small: out.append("routes, bound+n <= LP")
        if not small and n <= LP: out.append("routes, bound+n > LP")
        if zero: out.append("routes, count 0")
    if 33 <= n <= 64: out.append("n 33..64")
    if n > 64: out.append("n > 64")
    return out


class Census:
    """the census of a batch, folded into the buckets the tests assert on"""

    def __init__(self, per_graph, classes, g_nv, K):
        self.fans = {}; self.fans_by_group = {}; self.routers = {}; self.K = K
        for g, cen in enumerate(per_graph):
            grp = class_group(int(classes[g]), int(g_nv[g]), K)
            for key, n in cen.items():
                if key[0] == 0:
                    d = "out" if key[1] == 0 else "in"; fb = fan_bucket(key[2], K)
                    self.fans[(fb, d)] = self.fans.get((fb, d), 0) + n
                    if 2 <= key[2] <= 8:
                        self.fans_by_group[(fb, d, grp)] = self.fans_by_group.get((fb, d, grp), 0) + n
                else:
                    for b in router_buckets(key, K):
                        self.routers[b] = self.routers.get(b, 0) + n

    def router_names(self):
        LP = self.K["LP"]
        return ["2+2 plain", "2+2 routes or samples"] + ["n=%d no routes" % x for x in (LP - 1, LP, LP + 1)] + \
               ["small, several samples", "small, table", "largest small, no routes", "smallest large, no routes",
                "routes, bound+n <= LP", "routes, bound+n > LP", "routes, count 0", "n 33..64", "n > 64"]

    def required(self):
        """every bucket the hub batch must fill: name -> events"""
        out = {}
        for fb in fan_buckets(self.K):
            for d in ("in", "out"):
                if fb == "1" and d == "in": continue        # a vertex with one edge on each side is taken as an out-fan (the dispatch tests nin == 1 first)
                out["fan %s %s" % (fb, d)] = self.fans.get((fb, d), 0)
        for fb in ("2", "3", "4", "5-8"):
            for d in ("in", "out"):
                for grp in ("0-1", "2-9", "twins", "10,13"):
                    out["fan %s %s class %s" % (fb, d, grp)] = self.fans_by_group.get((fb, d, grp), 0)
        for b in self.router_names():
            out["router " + b] = self.routers.get(b, 0)
        return out

    def required_of_group(self, grp: str):
        """the lines of required() that belong to one class group"""
        return {k: v for k, v in self.required().items() if k.endswith(" class " + grp)}

    def add_group(self, other: "Census", grp: str):
        """the fans of ONE class group of another census, nothing else of it (tests/class_cases.py fills the group of classes 10 / 13 with
        small hubs that are run in those classes; the other lines stay what the hub batch alone gives)"""
        for k, v in other.fans_by_group.items():
            if k[2] == grp: self.fans_by_group[k] = self.fans_by_group.get(k, 0) + v
        return self

    def add(self, other: "Census"):
        for mine, theirs in ((self.fans, other.fans), (self.fans_by_group, other.fans_by_group), (self.routers, other.routers)):
            for k, v in theirs.items(): mine[k] = mine.get(k, 0) + v
        return self

    def table(self) -> str:
        return "\n".join("%-40s %6d" % kv for kv in self.required().items())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------------------------------------------------
FANS = (1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 48, 63, 64, 65, 100, 300)
ROUTERS = ((2, 2), (2, 3), (3, 3), (3, 4), (4, 4), (5, 6), (6, 6), (6, 7), (7, 8), (8, 8), (8, 9), (9, 9), (20, 20), (33, 33), (40, 40), (70, 5), (5, 70))
CHUNK_EDGES = (62, 63, 64, 65, 127, 128, 129)
REPEAT = 12            # copies (with their own draws) of every degree: the census asks for 10 events a bucket


def star_graphs(seed: int = 20240, fans=FANS, repeat=REPEAT):
    """single hubs, alone: every fan size in both directions, every switch in turn"""
    rng = np.random.default_rng(seed); out = []
    modes = ("random", "tied", "remainder", "deficit", "tied_int")
    for k in fans:
        for out_dir in (True, False):
            for r in range(repeat):
                same = (2 + r % 2) if (r % 4 == 1 and k >= 3) else 0
                g = star(rng, k, out_dir, same_target=same, to_sink=(2 if (r % 6 == 2 and k >= 4) else 0), weights=modes[r % len(modes)],
                         samples=1 + r % 4, phasing=(r % 3 == 0), strand=(0, 1, 2)[r % 3] if r % 2 else 0, stem=(r % 2 == 0))
                g["strand"] = "+-."[r % 3]
                out.append(lay_out(g, rng))
    return out


def star_graphs_with_tails(seed: int = 20241, fans=FANS, repeat=REPEAT):
    """the same hubs with a random tail (class 0 / 1 up to k = 8, larger classes beyond) and, for fans of 2..8, padded into classes 2..9"""
    rng = np.random.default_rng(seed); out = []
    modes = ("random", "tied", "tied_int", "remainder")
    for k in fans:
        for out_dir in (True, False):
            for r in range(repeat):
                base = synth_base(int(rng.integers(1, 1 << 30)), int(rng.integers(8, 16)), 2, weight_mode=r % 3, n_samples=1 + r % 3, phasing_per_graph=(3 if r % 2 else 0))
                g = star(rng, k, out_dir, base=base, weights=modes[r % len(modes)], samples=1 + r % 3, phasing=(r % 2 == 1), same_target=(2 if (r % 5 == 3 and k >= 3) else 0))
                out.append(lay_out(g, rng))
            if k <= 8:
                for r in range(repeat):
                    base = synth_base(int(rng.integers(1, 1 << 30)), int(rng.integers(70, 250)), 3, weight_mode=r % 3, phasing_per_graph=(4 if r % 2 else 0))
                    g = star(rng, k, out_dir, base=base, weights=modes[r % len(modes)], samples=1 + r % 2, phasing=(r % 2 == 1))
                    out.append(lay_out(g, rng))
    return out


def router_graphs(seed: int = 20242, routers=ROUTERS, repeat=REPEAT):
    """k_in x k_out hubs: random and tied weights, with and without routes, one sample or several, alone and with a tail"""
    rng = np.random.default_rng(seed); out = []
    for kin, kout in routers:
        for r in range(2 * repeat):
            base = None if r % 3 else synth_base(int(rng.integers(1, 1 << 30)), int(rng.integers(8, 20)), 2, weight_mode=r % 3)
            routes = (r % 4 >= 2)
            g = router(rng, kin, kout, base=base, weights=("tied" if r % 2 else "random"), samples=(1 if r % 8 < 5 else 3), phasing=routes, guard=(r % 6 != 5))
            out.append(lay_out(g, rng))
    return out


def embedded_hub_graphs(seed: int = 20243, where=CHUNK_EDGES):
    """hubs spliced into a synth graph so that the hub's vertex index sits on either side of a 64-vertex chunk edge of the sweeps"""
    rng = np.random.default_rng(seed); out = []
    for idx in where:
        for r, k in enumerate((2, 3, 4, 5, 8, 33)):
            for out_dir in (True, False):
                base = synth_base(int(rng.integers(1, 1 << 30)), idx + 30 + k, 3, weight_mode=1)           # integer weights: ties between vertices
                g = star(rng, k, out_dir, base=base, hub_index=idx, weights="tied_int", phasing=False)
                out.append(lay_out(g, rng))
        for kin, kout in ((2, 2), (3, 3)):
            base = synth_base(int(rng.integers(1, 1 << 30)), idx + 40, 3, weight_mode=1)
            out.append(lay_out(router(rng, kin, kout, base=base, hub_index=idx, weights="tied"), rng))
    return out


def twin_graphs(seed: int = 20244, n: int = 24):
    """graphs of twin size (385..512 vertices): a synth graph with several small hubs (fans of 2..8, both directions, and 2 x 2 / 3 x 3 routers)"""
    rng = np.random.default_rng(seed); out = []
    for r in range(n):
        g = synth_base(int(rng.integers(1, 1 << 30)), int(rng.integers(330, 400)), 3, weight_mode=r % 3, phasing_per_graph=(5 if r % 2 else 0), n_samples=1 + r % 2)
        for k in (2, 3, 4, 5, 6, 8):
            for out_dir in (True, False):
                g = star(rng, k, out_dir, base=g, weights=("random", "tied", "tied_int")[(r + k) % 3], samples=1 + r % 2, same_target=(2 if (r + k) % 4 == 0 and k >= 3 else 0))
        g = router(rng, 2 + r % 2, 2 + r % 2, base=g, weights="tied" if r % 2 else "random")
        assert 385 <= g["V"] <= 512, g["V"]
        out.append(lay_out(g, rng))
    return out


def zero_count_graphs(seed: int = 20245, repeat=REPEAT):
    """hubs with an edge whose edge_info.count is 0 (router.cc:269 treats it as absent; a merge of it is one of the reference's asserts):
    kept apart from hub_batch(), whose graphs all end with status 0"""
    rng = np.random.default_rng(seed); out = []
    for kin, kout in ((2, 2), (2, 3), (3, 3), (3, 4), (2, 6)):
        for r in range(repeat):
            out.append(lay_out(router(rng, kin, kout, phasing=True, zero_count=True, samples=1 + r % 2, weights=("tied" if r % 2 else "random")), rng))
    for k in (2, 3, 4, 5, 9, 33):
        for out_dir in (True, False):
            for r in range(3):
                out.append(lay_out(star(rng, k, out_dir, zero_count=True, weights=("tied" if r % 2 else "random")), rng))
    return out


_CACHE = {}


def hub_batch(without=()):
    """the batch of both tiers -> (PackedGraphs, list of graph dicts); without: generator names left out (the census test's self-check)"""
    key = tuple(sorted(without))
    if key not in _CACHE:
        parts = dict(star=star_graphs, star_tail=star_graphs_with_tails, router=router_graphs, embedded=embedded_hub_graphs, twin=twin_graphs)
        graphs = []
        for name, fn in parts.items():
            if name in without: continue
            if name in ("star", "star_tail") and any(isinstance(w, int) for w in without):
                graphs += fn(fans=tuple(k for k in FANS if k not in without))
            else:
                graphs += fn()
        rng = np.random.default_rng(977)
        permute = set(int(i) for i in np.nonzero(rng.random(len(graphs)) < 0.3)[0])
        _CACHE[key] = (pack(graphs, rng, permute), graphs)
    return _CACHE[key]


def wide_router_params():
    """Parameters under which a wide hub WITHOUT phasing lists reaches the router at all.  With the defaults the smallest-edge rule (ratio
    min / sum <= 0.30, scallop.cc:844-945) fires before the router on every vertex with four or more edges on a side -- its guards only hold
    back edges whose far end has no other edge, and such a far end is a trivial vertex that was merged away earlier -- so a router of more
    than about seven edges is only ever built where phasing paths protect the edges.  A ratio of 0 leaves that rule its `< 0.01` branch."""
    p = A.default_params(); p.max_decompose_error_ratio[0] = 0.0
    return p


def wide_router_graphs(seed: int = 20246, routers=ROUTERS, repeat=REPEAT):
    """k_in x k_out hubs without any phasing list in the graph, for wide_router_params(): router_small up to its arena limit, router_large beyond"""
    rng = np.random.default_rng(seed); out = []
    K = kernel_constants(); extra = []
    for n in range(5, K["LP"] + 3):                       # every size up to and around LP, split evenly: the arena limit lies somewhere in there
        extra.append((n // 2, n - n // 2))
    for kin, kout in tuple(routers) + tuple(extra):
        for r in range(repeat):
            base = None if r % 3 else synth_base(int(rng.integers(1, 1 << 30)), int(rng.integers(8, 20)), 2, weight_mode=r % 3)
            g = router(rng, kin, kout, base=base, weights=("tied" if (r % 2 or kin + kout > 30) else "random"), samples=(1 if r % 4 < 3 else 3), guard=(r % 6 != 5))
            out.append(lay_out(g, rng))
    return out


def wide_router_batch():
    """-> (PackedGraphs, graph dicts, parameters)"""
    if "wide" not in _CACHE:
        graphs = wide_router_graphs()
        _CACHE["wide"] = (pack(graphs, np.random.default_rng(979), set(range(0, len(graphs), 4))), graphs, wide_router_params())
    return _CACHE["wide"]


def zero_count_batch():
    if "zero" not in _CACHE:
        graphs = zero_count_graphs()
        _CACHE["zero"] = (pack(graphs, np.random.default_rng(978), ()), graphs)
    return _CACHE["zero"]


def raw_form(g: dict):
    """a hub graph as the raw entry point takes it: (single-graph PackedGraphs, phases as exon-coordinate lists with their counts)"""
    phases = []
    for v, c in g["phasing"]:
        co = []
        for a in v:
            if co and co[-1] == g["lpos"][a]: co[-1] = g["rpos"][a]
            else: co += [g["lpos"][a], g["rpos"][a]]
        phases.append((co, c))
    pg = pack([dict(g, phasing=[])])
    return pg, phases
