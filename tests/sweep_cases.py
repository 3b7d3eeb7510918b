"""Hand-made graphs that put ties, exact thresholds and chosen lane positions in front of the three wave-parallel selections of the rule
cascade (decomp_device.h: scan_trivial, the selection loop of sweep_smallest_body, sweep_unsplittable; decomp_common.h: wave_argmin), for
tests/test_sweep_ties_cpu.py and tests/test_sweep_ties_gpu.py.

The single-lane emulation does not run wave_argmin (an empty stub where ALD_WAVE == 1) nor the interplay of the lanes (`lim`, a stop lane in
front of a now lane, the per-lane fold over the chunks), so those decisions are checked on the GPU only -- and, before this file, only by what
the random mixes happened to hit.  Two graph families make every such decision on purpose:

  comb    source -> tooth -> sink, one tooth per vertex, in-weight a, out-weight b: every tooth is a type-1 trivial vertex of balance ratio
          max(a / b, b / a); 51 / 50 and 102 / 100 are exactly the double 1.02, 30 / 20 exactly 1.5.  A `chain` is two teeth in a row
          (source -> u -> t -> sink): type 1 for resolve_trivial_vertex_fast as well, which classifies without the dominate query.
  block   a (parallel in-edges from the source) -> x1, x2 -> z (parallel out-edges to the sink): once the trivial x vertices are gone, a and z
          are smallest-edge candidates of ratio min / sum of their parallel side; (3, 7) is exactly 0.3, (2, 8) exactly 0.2, (1, 99) exactly 0.01.

A graph is a sequence of such pieces at chosen vertex indices, the gaps filled with teeth of ratio 1.0 (they all go in the first sweep) or of
distinct ratios above every threshold.  On top of them: a batch of random graphs under parameter sets that move what no other test moves
(max_decompose_error_ratio[4] / [5], min_guaranteed_edge_weight, and the four indices the kernel does not read), and single graphs of that batch
run with a threshold set to exactly a ratio of their own default trace, to the double below it and to the double above.

census() counts what all of this exercised FROM THE ORACLE ALONE (its second census map, scallop_oracle.hpp: SweepCensus, and its op traces):
a condition on the inputs, asserted in both tiers at MIN_EVENTS a line."""
from __future__ import annotations

import ctypes as C

import numpy as np

import aletsch_amd as A
from aletsch_amd.packed import PackedGraphs, export_via
import class_cases as CC
import common
import device_run as DR
import shapes

MIN_EVENTS = 10
MIN_POSITIONS = 120                      # line (a): distinct (chunk, lane) winner positions ...
MUST_POSITIONS = [(0, l) for l in (1, 15, 16, 31, 32, 47, 48, 63)] + [(1, 0), (1, 63)]      # ... these among them
REPEAT = 10                              # graphs per bullet (one event of the bullet's kind each, or more)
TRACE_CAP = 1 << 12
N_PARAM_GRAPHS = 120
N_DERIVED = 12                           # trace-derived events per kind
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the parameter sets
# ---------------------------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    p = A.default_params()
    for k, v in kw.items():
        if k == "minw": p.min_guaranteed_edge_weight = v
        else: p.max_decompose_error_ratio[int(k[1:])] = v
    return p


def param_sets():
    """name -> parameters (None: the default).  `unread` moves only the indices the kernel does not read (1, 2, 3, 6): the oracle's results
    under it must be the default's."""
    return {"default": None, "second": CC.second_params(), "jump15": _params(r7=1.5),
            "single005": _params(r5=0.05), "single09": _params(r5=0.9), "pure005": _params(r4=0.05), "pure02": _params(r4=0.2),
            "minw05": _params(minw=0.5), "minw10": _params(minw=1.0), "minw20": _params(minw=2.0),
            "unread": _params(r1=0.4, r2=0.5, r3=2.5, r6=0.7)}


CASE_SETS = ("default", "second", "jump15")                                                    # the hand-made cases run under these
VARIED = ("single005", "single09", "pure005", "pure02", "minw05", "minw10", "minw20")          # the random batch runs under these (+ default, unread)


# ---------------------------------------------------------------------------------------------------------------------------------------
# pieces -> graph
# ---------------------------------------------------------------------------------------------------------------------------------------
def tooth(a, b): return ("tooth", float(a), float(b))
def chain(a, b, c): return ("chain", float(a), float(b), float(c))
def block(ins, mids, outs): return ("block", [float(x) for x in ins], [float(x) for x in mids], [float(x) for x in outs])


_SIZE = {"tooth": 1, "chain": 2, "block": 4}


def flat(rng): w = int(rng.integers(5, 40)); return tooth(w, w)              # filler of ratio 1.0: taken `now` in the first sweep


def high(j): return tooth(300 + j, 100)                                       # filler of ratio 3.0 + j / 100: above every threshold, all distinct


def assemble(placed: dict, rng, filler, n_min: int = 0) -> dict:
    """placed: first vertex -> piece; every other vertex up to the last piece (and up to n_min inner vertices) is filler(k) (k-th filler)"""
    edges = []; v = 1; k = 0; last = max(max(s + _SIZE[p[0]] for s, p in placed.items()), n_min + 1); seq = []
    while v < last:
        p = placed.get(v)
        if p is None:
            p = filler(k); k += 1
            assert p[0] == "tooth"
        for q in range(v + 1, v + _SIZE[p[0]]): assert q not in placed, (v, q)
        seq.append((v, p)); v += _SIZE[p[0]]
    V = v + 1; sink = V - 1
    assert V <= 200
    E = lambda s, t, w: edges.append([s, t, w, 0, {0: w}])
    for s, p in seq:
        if p[0] == "tooth": E(0, s, p[1]); E(s, sink, p[2])
        elif p[0] == "chain": E(0, s, p[1]); E(s, s + 1, p[2]); E(s + 1, sink, p[3])
        else:
            for w in p[1]: E(0, s, w)
            E(s, s + 1, p[2][0]); E(s, s + 2, p[2][1]); E(s + 1, s + 3, p[2][0]); E(s + 2, s + 3, p[2][1])
            for w in p[3]: E(s + 3, sink, w)
    return shapes.lay_out(dict(V=V, edges=edges, vw=[0.0] * V, phasing=[], strand="."), rng)


def comb(pairs, rng): return assemble({1 + i: tooth(a, b) for i, (a, b) in enumerate(pairs)}, rng, None)


def cand_a(ins, s=None):
    """a block whose `a` is the candidate (ratio min(ins) / sum(ins)); its z stays at 0.5"""
    s = sum(ins) if s is None else s
    return block(ins, (s / 2, s / 2), (s / 2, s / 2))


def cand_z(outs):
    """a block whose `z` is the candidate; its a stays at 0.5"""
    s = sum(outs); return block((s / 2, s / 2), (s / 2, s / 2), outs)


# the positions of the tie bullets of (c) and (f): name -> vertex sets for groups of 2, 3 and 5 (a straddle is always a pair)
def _tie_positions(r: int):
    v = 3 + 4 * (r % 12)
    return {"in one chunk": ((v, v + 9), (v, v + 5, v + 13), (v, v + 4, v + 8, v + 12, v + 16)),
            "in the same lane of two chunks": ((v, v + 64), (v, v + 64, v + 128), (v, v + 4, v + 64, v + 68, v + 128)),
            "in different lanes of different chunks": ((v, v + 73), (v, v + 77, v + 137), (v, v + 5, v + 77, v + 90, v + 139)),
            "across vertices 63 | 64": ((63, 64),) * 3, "across vertices 127 | 128": ((127, 128),) * 3}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the families -> [(label, parameter set, graph dict)]
# ---------------------------------------------------------------------------------------------------------------------------------------
def comb_cases():
    rng = np.random.default_rng(5101); out = []
    # (a) winner positions: distinct ratios from exactly 1.02 up, in a seeded random order; every turn of the cascade is one wave_argmin
    for n in (126, 130):
        out.append(("a", "default", comb([(102 + int(j), 100) for j in rng.permutation(n)], rng)))
    # (b) ratios that share their upper 32 bits: 1.5 + k * 2^-30
    for n in (126, 130):
        out.append(("b", "default", comb([(3 * 2 ** 29 + int(k), 2 ** 30) for k in rng.permutation(1024)[:n]], rng)))
    # (c) ties at the minimum
    for r in range(REPEAT):
        for name, groups in _tie_positions(r).items():
            pos = groups[r % 3]; a = 110 + r
            out.append(("c " + name, "default", assemble({p: tooth(a, 100) for p in pos}, rng, lambda k: flat(rng))))
    # (d) ratio exactly 1.02 (51 / 50, 102 / 100), and a `now` tooth (101 / 100) around it
    for r in range(REPEAT):
        exact = tooth(51, 50) if r % 2 else tooth(100, 102); now = tooth(101, 100); v = 2 + 5 * r
        out.append(("d alone", "default", assemble({v: exact}, rng, high)))
        out.append(("d in front of now, same chunk", "default", assemble({v: exact, v + 7: now}, rng, high)))
        out.append(("d in front of now, other chunk", "default", assemble({v: exact, v + 64 + r: now}, rng, high)))
        out.append(("d behind now, same chunk", "default", assemble({v: now, v + 7: exact}, rng, high)))
        out.append(("d behind now, other chunk", "default", assemble({v: now, v + 64 + r: exact}, rng, high)))
    # (e) jump_ratio = 1.5
    for r in range(REPEAT):
        v = 2 + 5 * r; stop = tooth(120 + r, 100); now = tooth(101, 100)
        out.append(("e exactly jump_ratio", "jump15", assemble({v: tooth(30, 20), v + 3: tooth(45, 30)}, rng, high, n_min=70 if r % 2 else 0)))
        out.append(("e exactly 1.02 stops", "jump15", assemble({v + 4: tooth(51, 50) if r % 2 else tooth(102, 100)}, rng, high, n_min=v + 20)))
        out.append(("e stop in front of now, same chunk", "jump15", assemble({v: stop, v + 7: now}, rng, high)))
        out.append(("e stop in front of now, other chunk", "jump15", assemble({v: stop, v + 64 + r: now}, rng, high)))
        out.append(("e stop behind now, same chunk", "jump15", assemble({v: now, v + 7: stop}, rng, high)))
        out.append(("e stop behind now, other chunk", "jump15", assemble({v: now, v + 64 + r: stop}, rng, high)))
        out.append(("e fast at exactly jump_ratio", "jump15", assemble({v: chain(30, 20, 20), v + 4: chain(60, 40, 40)}, rng, high, n_min=v + 10)))
        out.append(("e fast at 1.2", "jump15", assemble({v: chain(24, 20, 20), v + 66: chain(12, 10, 10)}, rng, high)))
    return out


def block_cases():
    rng = np.random.default_rng(5201); out = []
    # (f) ties at the minimum between 2, 3 and more blocks
    for r in range(REPEAT):
        for name, groups in _tie_positions(r).items():
            pos = groups[r % 3]; ins = (2 + r % 3, 18 - r % 3)           # 0.1, 0.15, 0.2
            placed = {}
            for p in pos:
                if p in (63, 127): placed[p - 3] = cand_z(ins)           # the z of a block that ends at the chunk edge ...
                else: placed[p] = cand_a(ins)                            # ... against the a of the block that begins behind it
            out.append(("f " + name, "default", assemble(placed, rng, lambda k: flat(rng))))
    # (g) threshold ties
    for r in range(REPEAT):
        v = 1 + 3 * r; k = 1 + r % 4
        out.append(("g exactly the threshold, default", "default", assemble({v: cand_a((3 * k, 7 * k)), v + 70: cand_a((4 * k, 6 * k))}, rng, lambda k: flat(rng))))
        out.append(("g exactly the threshold, second set", "second", assemble({1 + r % 8: cand_a((2 * k, 8 * k)), 12 + r % 8: cand_a((3 * k, 7 * k))}, rng, lambda k: flat(rng))))
        exact = cand_a((k, 99 * k)); now = cand_a((k, 199 * k)); other = cand_a((2, 8))
        out.append(("g 0.01 in front of now, same chunk", "default", assemble({v: exact, v + 8: now, v + 16: other}, rng, lambda k: flat(rng))))
        out.append(("g 0.01 in front of now, other chunk", "default", assemble({v: exact, v + 5: other, v + 80: now}, rng, lambda k: flat(rng))))
        out.append(("g 0.01 behind now, same chunk", "default", assemble({v: now, v + 8: other, v + 16: exact}, rng, lambda k: flat(rng))))
        out.append(("g 0.01 behind now, other chunk", "default", assemble({v: other, v + 5: now, v + 80: exact}, rng, lambda k: flat(rng))))
    # (h) ratios that share their upper 32 bits: 0.25 + k * 2^-30
    for n in (16, 40):
        ks = rng.permutation(1024)[:n]
        out.append(("h", "default", assemble({1 + 4 * i: cand_a((2 ** 28 + int(k), 3 * 2 ** 28 - int(k))) for i, k in enumerate(ks)}, rng, lambda k: flat(rng))))
    # (i) inside one vertex
    for r in range(REPEAT):
        v = 1 + 6 * r; k = 1 + r % 3
        out.append(("i two minimal in-edges", "default", assemble({v: cand_a((2 * k, 2 * k, 6 * k)), v + 66: cand_a((3, 3, 3, 21))}, rng, lambda k: flat(rng))))
        out.append(("i r1 == r2", "default", assemble({v: block((5 * k, 5 * k), (3 * k, 7 * k), (3 * k, 7 * k))}, rng, lambda k: flat(rng))))
    return out


def case_batch(name: str):
    """the hand-made cases that run under parameter set `name` -> (PackedGraphs, labels)"""
    if "cases" not in _CACHE:
        _CACHE["cases"] = comb_cases() + block_cases()
    mine = [(lab, g) for lab, s, g in _CACHE["cases"] if s == name]
    return shapes.pack([g for _, g in mine]), [lab for lab, _ in mine]


def param_batch() -> PackedGraphs:
    """random graphs on which the unsplittable passes decide"""
    if "param" not in _CACHE:
        _CACHE["param"] = A.synth(seed=5301, n_graphs=N_PARAM_GRAPHS, v_min=20, v_max=60, edges_per_vertex=4, phasing_per_graph=6, weight_mode=2, n_samples=2)
    return _CACHE["param"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle: results, op traces and the census of the sweeps
# ---------------------------------------------------------------------------------------------------------------------------------------
def oracle_full(pg: PackedGraphs, params=None):
    """-> dict(res, iters, traces, sweeps = per graph {13-field key: events} (scallop_oracle.hpp: SweepCensus))"""
    O = common.oracle_lib(); h = C.c_void_p()
    assert O.ora_run_packed(*pg.c_args(), C.byref(params) if params is not None else None, C.c_int32(CC.THREADS), C.c_int32(1), C.byref(h)) == 0
    res = export_via(O.ora_result_export, h, pg.n)
    st = np.zeros((pg.n, 6), np.int32); O.ora_result_stats(h, st.ctypes.data_as(C.POINTER(C.c_int32)))
    traces = []; sweeps = []
    for g in range(pg.n):
        n = C.c_int32(); O.ora_result_trace(h, g, C.byref(n), None, None, 0)
        codes = np.zeros(3 * max(n.value, 1), np.int32); vals = np.zeros(max(n.value, 1))
        O.ora_result_trace(h, g, C.byref(n), codes.ctypes.data_as(C.POINTER(C.c_int32)), vals.ctypes.data_as(C.POINTER(C.c_double)), n.value)
        traces.append([(int(codes[3 * i]), int(codes[3 * i + 1]), int(codes[3 * i + 2]), float(vals[i])) for i in range(n.value)])
        O.ora_result_sweep_census(h, C.c_int32(g), C.byref(n), None, C.c_int32(0))
        rows = np.zeros((max(n.value, 1), 14), np.int32)
        O.ora_result_sweep_census(h, C.c_int32(g), C.byref(n), rows.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(n.value))
        sweeps.append({tuple(int(x) for x in rows[i, :13]): int(rows[i, 13]) for i in range(n.value)})
    O.ora_result_free(h)
    assert max(len(t) for t in traces) <= TRACE_CAP
    return dict(pg=pg, params=params, res=res, iters=st[:, 3].copy(), traces=traces, sweeps=sweeps)


def runs():
    """everything both tiers run: name -> dict(pg, params, res, iters, traces, sweeps, labels or None), the oracle's answer computed once.
    `cases/<set>`: the hand-made cases; `param/<set>`: the random batch; `derived/<kind>/<k>/<at|below|above>`: one graph of it alone"""
    if "runs" in _CACHE:
        return _CACHE["runs"]
    P = param_sets(); out = {}
    for s in CASE_SETS:
        pg, labels = case_batch(s)
        out["cases/" + s] = dict(oracle_full(pg, P[s]), labels=labels)
    for s in ("default", "unread") + VARIED:
        out["param/" + s] = dict(oracle_full(param_batch(), P[s]), labels=None)
    # trace-derived ties: an event of the default trace, its graph alone, the rule's threshold set to exactly its ratio / the doubles around it
    base = out["param/default"]; pg = param_batch()
    kinds = {"smallest": (lambda e: e[0] == 6, 0), "unsplit single": (lambda e: e[0] == 8 and e[2] == 5 and e[3] > 0.01, 5),
             "unsplit pure": (lambda e: e[0] == 8 and e[2] == 4 and e[3] > 0.01, 4)}
    for kind, (pred, index) in kinds.items():
        # (an event is taken where the oracle's trace differs between `at` and `below`: elsewhere the same vertex only fires one pass later)
        k = 0
        for g, t in enumerate(base["traces"]):
            one = pg.select(np.array([g]))
            for ev in [e for e in t if pred(e) and np.isfinite(e[3]) and e[3] > 0][:4]:
                if k == N_DERIVED: break
                three = {}
                for where, val in (("at", ev[3]), ("below", float(np.nextafter(ev[3], 0.0))), ("above", float(np.nextafter(ev[3], np.inf)))):
                    p = A.default_params(); p.max_decompose_error_ratio[index] = val
                    three[where] = dict(oracle_full(one, p), labels=None)
                if three["at"]["traces"] == three["below"]["traces"]: continue
                for where, o in three.items(): out["derived/%s/%d/%s" % (kind, k, where)] = o
                k += 1; break
        assert k == N_DERIVED, (kind, k)
    _CACHE["runs"] = out
    return out


def batched_runs():
    """the runs of several graphs (cases/*, param/*)"""
    return {k: v for k, v in runs().items() if not k.startswith("derived/")}


def derived_runs():
    return {k: v for k, v in runs().items() if k.startswith("derived/")}


def emu_full(pg: PackedGraphs, params=None, force_class: int = 0, keep: bool = False):
    """one run of the single-lane emulation, every graph traced -> (DecompResult, iterations, classes, traces); keep: the build that keeps the
    sweep records in every class and aborts on a stale one"""
    E = common.emu_keep_lib() if keep else common.emu_lib(); h = C.c_void_p()
    rc = E.emu_run_packed(*pg.c_args(), C.byref(params) if params is not None else None, C.c_int32(TRACE_CAP), C.c_int32(force_class), C.byref(h))
    assert rc == 0, rc
    r = export_via(E.emu_result_export, h, pg.n)
    it = np.zeros(pg.n, np.int32); cl = np.zeros(pg.n, np.int32)
    E.emu_result_iters(h, it.ctypes.data_as(C.POINTER(C.c_int32)), cl.ctypes.data_as(C.POINTER(C.c_int32)))
    traces = [common.emu_trace_of(E, h, g, TRACE_CAP) for g in range(pg.n)]
    E.emu_result_free(h)
    return r, it, cl, traces


def natural_classes(name: str):
    """the class every graph of a run ends in without a first class, as the emulation's host policy finds it"""
    key = "natural_" + name
    if key not in _CACHE:
        o = runs()[name]; _CACHE[key] = common.emu_run(o["pg"], params=o["params"])[2]
    return _CACHE[key]


def expected_classes(name: str, first: int):
    return np.maximum(natural_classes(name), first)


def device_mismatches(name: str, first: int = 0, cls: int = 0):
    """run `name` through the library the process has loaded with the first class forced (cls: the class that stands for `first`, its twin or
    itself) -> device_run.oracle_mismatches per batch: the classes the graphs ran in, statuses, records and, for every graph that does not
    end on an invariant status, the iteration count and the whole op trace"""
    o = runs()[name]; pg = o["pg"]; bad = []
    want_cls = expected_classes(name, first).copy(); want_cls[want_cls == first] = cls
    for idx in DR.in_chunks(pg.n, cls):
        r = DR.run(pg if len(idx) == pg.n else pg.select(idx), o["params"], first=first, twin="1" if cls in DR.TWIN_OF else "0", trace_cap=TRACE_CAP)
        bad += DR.oracle_mismatches("%s from graph %d" % (name, idx[0]), r, common.select_results(o["res"], idx), o["iters"][idx], o["traces"],
                                    want_classes=DR.class_counts(want_cls[idx]), traced=idx, skip_failed=True)
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------------
RULE, END, NCAND, NTIED, WC, WL, LC, LL, MASK, SHARED, REL_EXACT, REL_STOP, INNER = range(13)
_REL = {"in front of now, same chunk": 1, "in front of now, other chunk": 2, "behind now, same chunk": 3, "behind now, other chunk": 4}


def _tie_kind(k):
    if k[LC] < 0: return None
    if (k[LC], k[LL], k[WC], k[WL]) == (0, 63, 1, 0): return "across vertices 63 | 64"
    if (k[LC], k[LL], k[WC], k[WL]) == (1, 63, 2, 0): return "across vertices 127 | 128"
    if k[LC] == k[WC]: return "in one chunk"
    return "in the same lane of two chunks" if k[LL] == k[WL] else "in different lanes of different chunks"


def _events(prefix: str, pred):
    """events of the sweep census, over the case graphs whose label starts with `prefix`, whose key satisfies pred"""
    n = 0
    for name, o in runs().items():
        if not name.startswith("cases/"): continue
        for lab, cen in zip(o["labels"], o["sweeps"]):
            if lab.startswith(prefix): n += sum(c for k, c in cen.items() if pred(k))
    return n


def winner_positions():
    """(chunk, lane) of every winner of a best-ended type-1 trivial sweep on the graphs of (a)"""
    pos = set()
    for o in (runs()["cases/default"],):
        for lab, cen in zip(o["labels"], o["sweeps"]):
            if lab == "a": pos |= {(k[WC], k[WL]) for k in cen if k[RULE] == 1 and k[END] == 3}
    return pos


def census():
    """name -> events (line (a): distinct winner positions), every line counted in the oracle"""
    if "census" in _CACHE:
        return _CACHE["census"]
    R = runs(); out = {}
    triv = lambda k: k[RULE] == 1
    small = lambda k: k[RULE] == 4
    out["a distinct winner positions (of %d asked)" % MIN_POSITIONS] = len(winner_positions())
    out["b argmin among ratios that share the upper word"] = _events("b", lambda k: triv(k) and k[END] == 3 and k[SHARED] == 1 and k[NCAND] >= 2)
    for fam, rule in (("c", triv), ("f", small)):
        for size, test in (("2", lambda n: n == 2), ("3", lambda n: n == 3), ("more than 3", lambda n: n > 3)):
            out["%s tie of %s at the minimum" % (fam, size)] = _events(fam + " ", lambda k: rule(k) and k[END] == 3 and test(k[NTIED]))
        for kind in _tie_positions(0):
            out["%s tie %s" % (fam, kind)] = _events("%s %s" % (fam, kind), lambda k: rule(k) and k[END] == 3 and k[NTIED] >= 2 and _tie_kind(k) == kind)
    out["d exactly 1.02 alone: taken as best"] = _events("d alone", lambda k: triv(k) and k[END] == 3 and k[MASK] & 1 and k[REL_EXACT] == 0)
    for name, rel in _REL.items():
        out["d exactly 1.02 " + name] = _events("d " + name, lambda k: triv(k) and k[END] == 1 and k[REL_EXACT] == rel)
    out["e exactly jump_ratio: a candidate, not a stop"] = _events("e exactly jump_ratio", lambda k: triv(k) and k[END] == 3 and k[MASK] & 2)
    out["e exactly 1.02 under jump_ratio 1.5: a stop"] = _events("e exactly 1.02", lambda k: triv(k) and k[END] == 2 and k[MASK] & 1)
    for name, rel in _REL.items():
        out["e stop " + name] = _events("e stop " + name, lambda k: triv(k) and k[REL_STOP] == rel and k[END] == (2 if rel <= 2 else 1))
    out["e fast pass refuses exactly jump_ratio"] = _events("e fast at exactly", lambda k: k[RULE] == 3 and k[MASK] & 8)
    out["e fast pass takes 1.2"] = _events("e fast at 1.2", lambda k: k[RULE] == 3 and k[MASK] & 16)
    out["g minimum exactly the threshold, default (0.3)"] = _events("g exactly the threshold, default", lambda k: small(k) and k[END] == 3 and k[MASK] & 2)
    out["g minimum exactly the threshold, second set (0.2)"] = _events("g exactly the threshold, second", lambda k: small(k) and k[END] == 3 and k[MASK] & 2)
    out["g exactly 0.01: taken as best, not now"] = _events("g 0.01", lambda k: small(k) and k[END] == 3 and k[MASK] & 1)
    for name, rel in _REL.items():
        out["g exactly 0.01 " + name] = _events("g 0.01 " + name, lambda k: small(k) and k[END] == 1 and k[REL_EXACT] == rel)
    out["h argmin among ratios that share the upper word"] = _events("h", lambda k: small(k) and k[END] == 3 and k[SHARED] == 1 and k[NCAND] >= 2)
    out["i two in-edges of the same minimal weight"] = _events("i two", lambda k: small(k) and k[END] == 3 and k[INNER] & 1)
    out["i r1 == r2 between the in and the out side"] = _events("i r1", lambda k: small(k) and k[END] == 3 and k[INNER] & 2)
    base = R["param/default"]["traces"]
    for s in VARIED:
        out["parameter %s: graphs whose trace differs from the default's" % s] = sum(1 for a, b in zip(R["param/" + s]["traces"], base) if a != b)
    for kind, rule in (("smallest", 4), ("unsplit single", 5), ("unsplit pure", 6)):
        out["derived %s: threshold at the ratio / the double below, traces differ" % kind] = \
            sum(1 for k in range(N_DERIVED) if R["derived/%s/%d/at" % (kind, k)]["traces"] != R["derived/%s/%d/below" % (kind, k)]["traces"])
        out["derived %s: a sweep's winner sits exactly on the threshold" % kind] = \
            sum(c for k in range(N_DERIVED) for key, c in R["derived/%s/%d/at" % (kind, k)]["sweeps"][0].items() if key[RULE] == rule and key[END] == 3 and key[MASK] & 2)
    _CACHE["census"] = out
    return out


def census_table() -> str:
    return "\n".join("%-75s %6d" % kv for kv in census().items())


def census_short():
    """the lines that miss what the issue of this file asks for"""
    cen = census(); short = {}
    for i, (k, v) in enumerate(cen.items()):
        if v < (MIN_POSITIONS if i == 0 else MIN_EVENTS): short[k] = v
    missing = [p for p in MUST_POSITIONS if p not in winner_positions()]
    if missing: short["a positions missing"] = missing
    return short
