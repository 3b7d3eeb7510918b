"""Small graphs for the extend of an unsplittable vertex with two in-edges and two out-edges (decomp_device.h: extend_22, the generic
decompose_vertex_extend beside it); tests/test_extend22_cpu.py and tests/test_extend22_gpu.py run them.

A graph is a lattice of up to six hubs between the source and the sink: every hub has exactly two in-edges and two out-edges (one hub may
have three on one side), so no trivial vertex stands in front of the unsplittable sweeps.  Weights are integer flows (every hub balanced:
the router's ratio is 0, OP_UNSPLIT_NOW), the same with the edges at the source and the sink perturbed (the inner hubs stay balanced), or
perturbed everywhere.  (Without sample sets or phasing paths the router splits a balanced-out hub with ratio 0 whatever the weights; the
OP_UNSPLIT_BEST case comes from hubs whose edges carry several samples.)  A chain of trivial vertices beside the lattice pads a graph to a vertex count and leaves a free
slot behind before the first extend.

What a batch is named for is asserted ON THE ORACLE'S OP TRACE: a graph belongs to a case when the trace has an OP_UNSPLIT_NOW / _BEST
event at a hub whose surroundings are still the input's at that moment -- every earlier event of the trace lies on the padding chain or
at a hub that shares no edge with it -- and the input has the named property at that hub.  batch(name) raises when no graph qualifies.

The trace names the vertex, not the pairs: which in-edge and which out-edge occur twice (i*, o*) is decided inside the router.  So the
three strand-borrow orders of the stranded batch and the phasing path through (i*, o*) that makes hs_insert_between act are counted
where they happen, by the counting build of the emulation (tests/test_extend22_cpu.py), each at least once.  raw_batch() hands the hubs
of three batches over in the raw form.

Not here: an in-edge and an out-edge of the root that share their far vertex.  The source of an in-edge precedes the root and the target
of an out-edge follows it in the vertex order of a splice graph, so no input reaches that state."""
from __future__ import annotations

import numpy as np

import aletsch_amd as A
import common
import shapes

OP_TRIVIAL = (2, 3, 4); OP_SMALL = (5, 6); OP_NOW, OP_BEST = 7, 8
MAX_GRAPHS = 512


def lattice(rng, k, perturb="none", wide=None, samples=1, phasing=False, strands=False, pad_to=None, p_source=0.4, topology=None):
    """k hubs (vertices 1..k), each 2 x 2; wide = (hub, "in" | "out"): that hub has three edges on that side; pad_to: a chain of trivial
    vertices source -> .. -> sink brings the graph to that many vertices; topology: "diamond" (k = 5: hub 3 between the distinct hubs 1, 2
    and 4, 5) "chain" (k = 3: hub 2 takes two parallel edges from hub 1 and sends two to hub 3) or "fork" (k = 3: hub 1 sends two parallel edges to
    the 3 x 2 hub 3, whose in-list holds a third edge from hub 2 BEHIND them: the pair moves past it) instead of a random lattice"""
    n_in = {i: 2 for i in range(1, k + 1)}; n_out = dict(n_in)
    if wide is not None: (n_in if wide[1] == "in" else n_out)[wide[0]] += 1
    free = {i: n_out[i] for i in range(1, k + 1)}
    pairs = []
    for i in range(1, k + 1):
        for _ in range(n_in[i]):
            avail = [u for u in range(1, i) if free[u] > 0]
            if avail and rng.random() > p_source:
                u = int(rng.choice(avail)); free[u] -= 1; pairs.append((u, i))
            else:
                pairs.append((0, i))
    sink = k + 1
    for u in range(1, k + 1):
        pairs += [(u, sink)] * free[u]
    if topology == "diamond": assert k == 5 and wide is None; pairs = [(0, 1), (0, 1), (0, 2), (0, 2), (1, 3), (2, 3), (1, 4), (2, 5), (3, 4), (3, 5), (4, 6), (4, 6), (5, 6), (5, 6)]
    if topology == "chain": assert k == 3 and wide is None; pairs = [(0, 1), (0, 1), (1, 2), (1, 2), (2, 3), (2, 3), (3, 4), (3, 4)]
    if topology == "fork": assert k == 3 and wide == (3, "in"); pairs = [(0, 1), (0, 1), (0, 2), (0, 2), (1, 3), (1, 3), (2, 3), (2, 4), (3, 4), (3, 4)]
    # integer flows.  A lattice of 2 x 2 hubs: the same base flow on every edge (two in, two out: conserved) plus a few source -> sink paths of
    # one to three units, so that the two edges of a side differ by little and the smallest-edge rule (min / sum <= 0.30) leaves the hubs
    # to the router.  With a wide hub: one path through every edge (run with wide_params(), which switch that rule off).
    ins = {v: [j for j, e in enumerate(pairs) if e[1] == v] for v in range(k + 2)}; outs = {v: [j for j, e in enumerate(pairs) if e[0] == v] for v in range(k + 2)}
    w = [0 if wide is not None else 20] * len(pairs)
    for j in (range(len(pairs)) if wide is not None else [int(x) for x in rng.integers(0, len(pairs), 4)]):
        path = [j]; v = pairs[j][0]
        while v != 0: e = int(rng.choice(ins[v])); path.append(e); v = pairs[e][0]
        v = pairs[j][1]
        while v != sink: e = int(rng.choice(outs[v])); path.append(e); v = pairs[e][1]
        f = int(rng.integers(1, 10 if wide is not None else 4))
        for e in path: w[e] += f
    V = k + 2 if pad_to is None else pad_to
    gs = int(rng.integers(1, 3))                         # the strand of the graph's stranded edges
    assert V >= k + 2
    mv = lambda x: V - 1 if x == sink else x
    edges = []
    for j, (s, t) in enumerate(pairs):
        wt = float(w[j])
        if perturb == "all" or (perturb == "ends" and (s == 0 or t == sink)): wt *= float(0.9 + 0.2 * rng.random())
        edges.append([s, mv(t), wt, (gs if rng.random() < 0.6 else 0) if strands else 0, shapes._samples(rng, wt, samples if samples == 1 else int(rng.integers(2, samples + 1)))])
    pads = list(range(k + 1, V - 1))
    if pads:
        wt = float(rng.integers(2, 20)); chain = [0] + pads + [V - 1]
        for a, b in zip(chain[:-1], chain[1:]): edges.append([a, b, wt, 0, {0: wt}])
    ph = []
    if phasing:
        for _ in range(int(rng.integers(1, 5))):
            mids = [v for v in range(1, k + 1) if any(pairs[e][0] != 0 for e in ins[v]) and any(pairs[e][1] != sink for e in outs[v])]
            if not mids: break
            v = int(rng.choice(mids))
            u = int(rng.choice([pairs[e][0] for e in ins[v] if pairs[e][0] != 0])); t = int(rng.choice([pairs[e][1] for e in outs[v] if pairs[e][1] != sink]))
            ph.append(([u, v, t], int(rng.integers(2, 9))))
    g = dict(V=V, edges=edges, vw=[0.0] * V, phasing=ph, strand="+-"[gs - 1] if strands else ".")
    g["k"] = k; g["wide"] = wide
    return shapes.lay_out(g, rng)


def _hub_facts(g, v, touched=()):
    """what the input says about hub v; touched: the hubs extended before it -- such a hub has been replaced by two new vertices, one per
    edge of a parallel pair, so a pair of edges it shares with v is no longer parallel (it is never the source or the sink)"""
    ein = [e for e in g["edges"] if e[1] == v]; eout = [e for e in g["edges"] if e[0] == v]; sink = g["V"] - 1
    shared = lambda ends: any(ends.count(x) > 1 and x not in touched for x in ends)
    return dict(nin=len(ein), nout=len(eout), par_in=shared([e[0] for e in ein]), par_out=shared([e[1] for e in eout]),
                src=any(e[0] == 0 for e in ein), snk=any(e[1] == sink for e in eout), multi=all(len(e[4]) >= 2 for e in ein + eout),
                strand=any(e[3] for e in ein + eout), routes=any(len(p) == 3 and p[1] == v for p, _ in g["phasing"]))


def _clean_events(g, trace):
    """the OP_UNSPLIT events of a trace at the input's hubs, up to the first event that changes a hub in another way:
    [(position, code, hub, facts of the hub, earlier events freed a slot)]"""
    k = g["k"]; touched = set(); out = []; freed = False
    for pos, (code, a, b, val) in enumerate(trace):
        if code in (OP_NOW, OP_BEST):
            if not (1 <= a <= k) or a in touched: break  # an extend at a vertex that is not the input's: nothing after it is the input's either
            out.append((pos, code, a, _hub_facts(g, a, touched), freed)); touched.add(a)
        elif code in OP_TRIVIAL and a > k: freed = True  # the padding chain
        elif code in OP_TRIVIAL + OP_SMALL: break
    return out


# name -> (generator options, predicate over (graph, clean events, facts of each event's hub))
def _any(pred): return lambda g, ev: any(pred(code, f, freed) for _, code, v, f, freed in ev)
def _is22(f): return f["nin"] == 2 and f["nout"] == 2
CASES = {
    "a_now": (dict(perturb="ends", k=(5, 5), topology="diamond"), _any(lambda c, f, fr: c == OP_NOW and _is22(f) and not (f["par_in"] or f["par_out"] or f["src"] or f["snk"]))),
    "a_best": (dict(perturb="all", k=(1, 5), samples=4), _any(lambda c, f, fr: c == OP_BEST and _is22(f))),
    "b_parallel_in": (dict(perturb="ends", k=(3, 3), topology="chain"), _any(lambda c, f, fr: _is22(f) and f["par_in"])),
    "b_parallel_out": (dict(perturb="ends", k=(3, 3), topology="chain"), _any(lambda c, f, fr: _is22(f) and f["par_out"] and not f["snk"])),
    "b_parallel_past_a_third": (dict(perturb="all", k=(3, 3), topology="fork", wide=True), _any(lambda c, f, fr: _is22(f) and f["par_out"] and not f["snk"])),
    "c_far_source": (dict(perturb="none", k=(1, 4)), _any(lambda c, f, fr: _is22(f) and f["src"])),
    "c_far_sink": (dict(perturb="none", k=(1, 4)), _any(lambda c, f, fr: _is22(f) and f["snk"])),
    "e_multi_sample": (dict(perturb="none", k=(1, 5), samples=4), _any(lambda c, f, fr: _is22(f) and f["multi"])),
    "f_phasing": (dict(perturb="none", k=(3, 6), phasing=True, p_source=0.2), _any(lambda c, f, fr: _is22(f) and f["routes"])),
    "g_strands": (dict(perturb="none", k=(1, 5), strands=True), _any(lambda c, f, fr: _is22(f) and f["strand"])),
    "h_slot_free_list": (dict(perturb="none", k=(1, 4), pad=(1, 4)), _any(lambda c, f, fr: _is22(f) and fr)),
    "h_slot_high_water": (dict(perturb="none", k=(1, 4)), _any(lambda c, f, fr: _is22(f) and not fr)),
    "i_63_vertices": (dict(perturb="none", k=(2, 5), pad_to=63), _any(lambda c, f, fr: _is22(f))),
    "i_64_vertices": (dict(perturb="none", k=(2, 5), pad_to=64), _any(lambda c, f, fr: _is22(f))),
    "j_wide_beside": (dict(perturb="none", k=(3, 6), wide=True),
                      lambda g, ev: any(_is22(f) for _, _, _, f, _ in ev) and any(f["nin"] + f["nout"] == 5 for _, _, _, f, _ in ev)),
    "k_two_now": (dict(perturb="none", k=(3, 6), p_source=0.7),
                  lambda g, ev: any(p2 == p1 + 1 and c1 == OP_NOW and c2 == OP_NOW and _is22(f1) and _is22(f2) for (p1, c1, _, f1, _), (p2, c2, _, f2, _) in zip(ev[:-1], ev[1:]))),
    "l_jump_ratio": (dict(perturb="none", k=(1, 5), jump=True), _any(lambda c, f, fr: _is22(f))),
}
CANDIDATES = 160
_CACHE = {}


def params_of(name):
    """the parameters a case runs with (None: the defaults)"""
    opt = CASES[name][0]
    if not (opt.get("jump") or opt.get("wide")): return None
    p = A.default_params()
    if opt.get("jump"): p.max_decompose_error_ratio[7] = 2.0
    if opt.get("wide"): p.max_decompose_error_ratio[0] = 0.0     # (the smallest-edge rule keeps its `< 0.01` branch: shapes.wide_router_params)
    return p


def batch(name):
    """-> (PackedGraphs, parameters or None, the oracle's (result, stats, traces), number of graphs that reach the case); raises when none does"""
    if name in _CACHE: return _CACHE[name]
    opt, pred = CASES[name]
    rng = np.random.default_rng(22000 + sorted(CASES).index(name)); graphs = []
    for r in range(CANDIDATES):
        k = int(rng.integers(opt["k"][0], opt["k"][1] + 1))
        wide = (int(rng.integers(1, k + 1)), "in" if r % 2 else "out") if opt.get("wide") else None
        if opt.get("topology") == "fork": wide = (3, "in")
        pad_to = opt.get("pad_to") or (k + 2 + int(rng.integers(opt["pad"][0], opt["pad"][1] + 1)) if opt.get("pad") else None)
        graphs.append(lattice(rng, k, perturb=opt["perturb"], wide=wide, samples=opt.get("samples", 1), phasing=opt.get("phasing", False), strands=opt.get("strands", False),
                              pad_to=pad_to, p_source=opt.get("p_source", 0.4), topology=opt.get("topology")))
    assert len(graphs) <= MAX_GRAPHS
    pg = shapes.pack(graphs); par = params_of(name)
    want, st, _, traces = common.oracle_run(pg, trace=True, params=par)
    hits = sum(1 for g, t in zip(graphs, traces) if pred(g, _clean_events(g, t)))
    assert hits > 0, "no graph of batch %r reaches its case in the oracle" % name
    _CACHE[name] = (pg, par, (want, st, traces), hits)
    _CACHE[name, "graphs"] = [g for g, t in zip(graphs, traces) if pred(g, _clean_events(g, t))]
    return _CACHE[name]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the raw form: the same lattices as the raw entry point takes them
# ---------------------------------------------------------------------------------------------------------------------------------------
RAW_CASES = ("a_now", "f_phasing", "g_strands")
RAW_GRAPHS = 48


def raw_ready(g, rng):
    """The raw entry point refuses parallel edges at the source and the sink (the reference's grouping is undefined on them), and every
    lattice has some.  Every further edge of such a group is led through a trivial vertex of its own (source -> x -> hub in front of the
    hubs, hub -> y -> sink behind them): the trivial rule merges x and y away before the first unsplittable sweep, and the router meets the
    lattice it would have met."""
    sink = g["V"] - 1; seen = set(); n_src = n_snk = 0
    for e in g["edges"]:
        key = (e[0], e[1])
        if (e[0] == 0 or e[1] == sink) and key in seen:
            if e[0] == 0: n_src += 1
            else: n_snk += 1
        seen.add(key)
    h = shapes.open_room(dict(g, count=None), 1, n_src) if n_src else dict(g, edges=[list(e) for e in g["edges"]])
    if n_snk: h = shapes.open_room(dict(h, count=None), h["V"] - 1, n_snk)
    sink = h["V"] - 1; x = 1; y = sink - n_snk; seen = set(); edges = []
    for e in h["edges"]:
        key = (e[0], e[1])
        if (e[0] == 0 or e[1] == sink) and key in seen:
            if e[0] == 0: edges += [[0, x] + list(e[2:]), [x, e[1]] + list(e[2:])]; x += 1
            else: edges += [[e[0], y] + list(e[2:]), [y, sink] + list(e[2:])]; y += 1
        else:
            edges.append(list(e))
        seen.add(key)
    out = dict(V=h["V"], edges=edges, vw=[0.0] * h["V"], phasing=h["phasing"], strand=g["strand"])
    return shapes.lay_out(out, rng)


def raw_batch(name):
    """the graphs of batch `name` that reach its case, made raw_ready -> (items for add_raw / emu_run_raw, the oracle's result and op traces
    on the graphs ITS pre-steps stage); asserts on that trace that every graph still has an OP_UNSPLIT event at a vertex with two
    in-edges and two out-edges in the staged graph's input"""
    if (name, "raw") in _CACHE: return _CACHE[name, "raw"]
    import ctypes as C
    from aletsch_amd.packed import PackedGraphs
    batch(name)
    O = common.oracle_lib()
    O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]; O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
    rng = np.random.default_rng(23000 + sorted(CASES).index(name)); items, staged = [], []
    for g in _CACHE[name, "graphs"][:RAW_GRAPHS]:
        pg, phases = shapes.raw_form(raw_ready(g, rng))
        want, _, _, rc = A.pre_assemble(pg, phases, 10000, _lib=O, _prefix="ora")
        assert rc == 0, (name, rc)
        items.append((pg, phases, 10000)); staged.append(want)
    spg = PackedGraphs.concat(staged)
    want, st, _, traces = common.oracle_run(spg, trace=True, params=params_of(name))
    assert (want.status == 0).all()
    reached = 0
    for i, t in enumerate(traces):
        one = shapes.unpack(spg, i); nin = {}; nout = {}
        for e in one["edges"]: nout[e[0]] = nout.get(e[0], 0) + 1; nin[e[1]] = nin.get(e[1], 0) + 1
        reached += any(c in (OP_NOW, OP_BEST) and a < one["V"] - 1 and nin.get(a) == 2 and nout.get(a) == 2 for c, a, b, v in t)
    assert reached >= len(items) // 2 and reached > 0, (name, reached, len(items))
    _CACHE[name, "raw"] = (items, spg, (want, st, traces))
    return _CACHE[name, "raw"]
