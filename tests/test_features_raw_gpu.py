"""GPU tier: ald_batch_features_all_ex with ALD_FEAT_RAW_ON_DEVICE -- raw graphs (as assembler::assemble(gx, px, sid) receives them) get their
feature rows from the device pass, which folds their boundaries into an overlay of the wire edges itself (trst_features_dev.h) -- against
the per-graph host routine ald_batch_features (which re-runs the pre-steps and re-stages each raw graph): row for row, field for field,
bit for bit, with the same per-graph return code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aletsch_amd as A
import common
from aletsch_amd.packed import PackedGraphs

pytestmark = pytest.mark.gpu

ROOT = common.ROOT


def _bits(rows, name):
    a = rows[name]
    return a.view(np.uint64) if a.dtype == np.float64 else a


def host_table(b, n, extras=None):
    """ald_batch_features graph by graph -> (rows, complete, rc per graph, row_begin)"""
    rows, comp, rcs, rb = [], [], [], [0]
    for g in range(n):
        f, c, rc = b.features(g, extras[g] if extras is not None else None)
        for x in f:
            rows.append(np.frombuffer(bytes(x), A.FEATURE_DTYPE)[0])
        comp.extend(c.tolist()); rcs.append(rc); rb.append(rb[-1] + len(f))
    return np.array(rows, A.FEATURE_DTYPE), np.array(comp, np.int32), np.array(rcs, np.int32), np.array(rb, np.int64)


def assert_tables_equal(got, want):
    rows, comp, rc, rb = want
    assert np.array_equal(got["row_begin"], rb)
    assert np.array_equal(got["graph_rc"], rc), np.nonzero(got["graph_rc"] != rc)[0][:10]
    assert np.array_equal(got["complete"], comp)
    keep = np.ones(len(comp), bool)
    for g in np.nonzero(rc != 0)[0]:                                  # the reference would have aborted there: partial values mean nothing
        keep[rb[g]:rb[g + 1]] = False
    for name in A.FEATURE_DTYPE.names:
        a, w = _bits(got["rows"], name)[keep], _bits(rows, name)[keep]
        assert np.array_equal(a, w), (name, np.nonzero(a != w)[0][:5])
    return int(keep.sum())


def random_extras(g_nv, rng):
    out = []
    for V in g_nv:
        V = int(V)
        out.append(A.GraphExtras.from_arrays(gr_reads=int(rng.integers(1, 10000)), gr_subgraph=int(rng.integers(0, 4)),
                                             boundary_loss1=rng.random(V), boundary_loss2=rng.random(V), boundary_loss3=rng.random(V), boundary_merged_loss=rng.random(V),
                                             unbridge_leaving_count=rng.integers(0, 9, V), unbridge_leaving_ratio=rng.random(V),
                                             unbridge_coming_count=rng.integers(0, 9, V), unbridge_coming_ratio=rng.random(V)))
    return out


def _oracle_pre():
    O = common.oracle_lib()
    O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]
    O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
    return O


def raw_item(g, phases, rng, dist):
    """graph dict -> (single-graph PackedGraphs, phases, dist) the way test_pre_steps_cpu.py hands it over: listing order = creation order"""
    pg = PackedGraphs.from_graphs([g])
    pg.edge_rank = np.array(sorted(range(len(g["edges"])), key=lambda k: (g["edges"][k][0], g["edges"][k][1])), np.int32)
    pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
    return pg, phases, dist


def raw_draw(seed, n_graphs, n_runs=(3, 10), keep_asserted=False):
    """the draw of the CPU tier (tests/test_features_raw_cpu.py): gene_like_raw graphs, dist from [10000, 10000, 150, 0]; graphs on which the
    oracle's pre-steps assert are left out (keep_asserted: ONLY those are returned) -> (items, number of folded boundaries)"""
    rng = np.random.default_rng(seed)
    O = _oracle_pre()
    items = []; folds = 0
    for t in range(n_graphs):
        g, phases = common.gene_like_raw(rng, n_runs=int(rng.integers(*n_runs)), strand="+-."[t % 3])
        it = raw_item(g, phases, rng, int(rng.choice([10000, 10000, 150, 0])))
        _, sm, tm, rc = A.pre_assemble(it[0], phases, it[2], _lib=O, _prefix="ora")
        if bool(rc) != keep_asserted:
            continue
        folds += 0 if rc else len(sm) + len(tm)
        items.append(it)
    return items, folds


def add_all_raw(b, items):
    for pg, phases, dist in items:
        assert b.add_raw(pg, phases, dist) == 0
    return [int(it[0].g_nv[0]) for it in items]


def run(b):
    b.upload(); b.run(); b.download()


def test_all_raw_batch_equals_the_host_routine(monkeypatch):
    items, folds = raw_draw(1078, 300)
    assert len(items) > 240 and folds > 100
    rng = np.random.default_rng(21)
    with A.DecompBatch(0) as b:
        g_nv = add_all_raw(b, items); n = len(items)
        run(b)
        ex = random_extras(g_nv, rng)
        got = b.features_all(ex, g_nv=g_nv, raw_on_device=True)
        st = got["stats"]
        assert st["host_graphs"] == 0 and st["device_graphs"] == n and st["device_ms"] > 0, st
        want = host_table(b, n, ex)
        rows = assert_tables_equal(got, want)
        assert rows > 500 and (got["complete"] == 1).sum() > 500
        ne_in = np.array([int(it[0].g_ne[0]) for it in items])
        fewer = [g for g in range(n) if got["row_begin"][g + 1] > got["row_begin"][g] and got["rows"]["gr_edges"][got["row_begin"][g]] < ne_in[g]]
        assert len(fewer) >= 30                                       # the grouped graphs are read, not the wire graphs
        monkeypatch.setenv("ALD_DEBUG_FEAT_LDS", "0")                 # every junction list in the scratch instead of LDS
        again = b.features_all(ex, g_nv=g_nv, raw_on_device=True)
        monkeypatch.delenv("ALD_DEBUG_FEAT_LDS")
        assert_tables_equal(again, want)
        assert again["stats"]["host_graphs"] == 0


def test_raw_and_staged_interleaved_flag_on_then_off():
    items, _ = raw_draw(1076, 75)
    items = items[:60]; assert len(items) == 60
    staged = A.synth(seed=33, n_graphs=60, v_min=8, v_max=60, edges_per_vertex=3, layout_mode=1, weight_mode=2)
    rng = np.random.default_rng(5)
    order = []
    with A.DecompBatch(0) as b:
        for t in range(120):
            if t % 2 == 0:
                pg, phases, dist = items[t // 2]
                assert b.add_raw(pg, phases, dist) == 0
                order.append(int(pg.g_nv[0]))
            else:
                one = staged.select(np.array([t // 2]))
                b.add(one); order.append(int(one.g_nv[0]))
        run(b)
        ex = [A.GraphExtras.from_arrays(gr_reads=int(rng.integers(1, 99)), boundary_loss2=rng.random(V), unbridge_leaving_ratio=rng.random(V)) for V in order]
        want = host_table(b, 120, ex)
        on = b.features_all(ex, g_nv=order, raw_on_device=True)
        assert on["stats"]["host_graphs"] == 0 and on["stats"]["device_graphs"] == 120
        assert assert_tables_equal(on, want) > 100
        off = b.features_all(ex, g_nv=order)                           # the same downloaded batch through the host routine
        assert off["stats"]["host_graphs"] == 60 and off["stats"]["device_graphs"] == 60
        assert_tables_equal(off, want)
        for name in A.FEATURE_DTYPE.names:
            assert on["rows"][name].tobytes() == off["rows"][name].tobytes(), name


def fan_graph(rng, width=70):
    """the 70-wide fans of the CPU tier: a run of `width` touching one-base vertices with a source edge to each, a few spliced exons, the
    mirror image into the sink; weights are not integers, so every sum depends on the order of its additions"""
    W = width
    lpos = [1000]; rpos = [1000]
    for i in range(W):
        lpos.append(1000 + i); rpos.append(1001 + i)
    mid = []
    pos = 1000 + W + 500
    for i in range(4):
        mid.append(len(lpos)); lpos.append(pos); rpos.append(pos + 120); pos += 120 + 300
    e0 = len(lpos)
    for i in range(W):
        lpos.append(pos + i); rpos.append(pos + i + 1)
    V = len(lpos) + 1; lpos.append(pos + W); rpos.append(pos + W)
    wt = lambda: float(rng.random() * 30 + 0.37)
    info = lambda: {0: float(rng.integers(1, 30)), int(rng.integers(1, 6)): float(rng.integers(1, 30))}
    edges = []
    add = lambda s, t, st=0: edges.append((s, t, wt(), st, info()))
    for i in range(1, W + 1):
        add(0, i)
    for i in range(1, W):
        add(i, i + 1)
    add(W, mid[0], 1); add(W // 2, mid[0], 1); add(W // 3, mid[1], 1); add(5, mid[0], 1)
    add(mid[0], mid[1], 1); add(mid[1], mid[2], 1); add(mid[0], mid[2], 1); add(mid[2], mid[3], 1); add(mid[1], mid[3], 1)
    add(mid[3], e0, 1); add(mid[2], e0 + W // 2, 1); add(mid[3], e0 + W // 3, 1); add(mid[1], e0 + W - 5, 1)
    for i in range(e0, e0 + W - 1):
        add(i, i + 1)
    for i in range(e0, e0 + W):
        add(i, V - 1)
    edges = [edges[i] for i in rng.permutation(len(edges))]
    vw = [0.0] + [float(rng.integers(1, 50)) for _ in range(V - 2)] + [0.0]
    g = dict(V=V, edges=edges, vw=vw, lpos=lpos, rpos=rpos, strand="+")
    phases = [([lpos[1], rpos[W], lpos[mid[0]], rpos[mid[0]]], 3), ([lpos[mid[2]], rpos[mid[2]], lpos[mid[3]], rpos[mid[3]]], 2)]
    return g, phases


def test_wide_fans_and_parallel_interior_edges():
    rng = np.random.default_rng(70)
    items = []
    for dist in (10000, 10000, 30, 0):
        g, phases = fan_graph(rng)
        items.append(raw_item(g, phases, rng, dist))
    n_fans = len(items)
    n_par = 0
    for t in range(150):                                              # duplicated interior edges: the newest LIVE parallel edge wins, the sums add every live one
        g, phases = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 10)), strand="+-."[t % 3])
        V = int(g["V"])
        dup = [e for e in g["edges"] if e[0] > 0 and e[1] < V - 1 and rng.random() < 0.25]
        g["edges"] = list(g["edges"]) + [(e[0], e[1], float(e[2]) * 0.5 + 1.3) + tuple(e[3:]) for e in dup]
        n_par += len(dup)
        items.append(raw_item(g, phases, rng, int(rng.choice([10000, 150]))))
    assert n_par > 100
    with A.DecompBatch(0) as b:
        g_nv = add_all_raw(b, items); n = len(items)
        run(b)
        ex = random_extras(g_nv, rng)
        got = b.features_all(ex, g_nv=g_nv, raw_on_device=True)
        want = host_table(b, n, ex)
        ok = want[2] == 0                                             # (a phase of the generator may make the pre-steps assert: those graphs have no paths
        keep = np.nonzero(ok)[0]                                      #  and the host routine reports the assert again; see test_invariant_graphs...)
        got_rc = got["graph_rc"].copy(); got_rc[~ok] = want[2][~ok]
        assert (got["graph_rc"][~ok] == 0).all() and (np.diff(got["row_begin"])[~ok] == 0).all()
        assert ok[:n_fans].all() and ok.sum() > 100
        assert_tables_equal(dict(got, graph_rc=got_rc), want) > 100
        rb = got["row_begin"]
        for g in range(2):                                            # dist 10000: 69 + 69 boundaries folded away
            assert rb[g + 1] > rb[g] and got["rows"]["gr_edges"][rb[g]] == int(items[g][0].g_ne[0]) - 138
        assert got["rows"]["gr_edges"][rb[3]] == int(items[3][0].g_ne[0])      # dist 0: nothing folds
        assert got["stats"]["host_graphs"] == 0


def test_large_raw_graphs_take_the_scratch_path():
    """gene_like_raw yields three long paths per graph whatever its size, so the junction lists (two words per internal vertex of every
    path) outgrow the 4096 LDS words only beyond a thousand vertices: n_runs = 520 gives V around 1300, the catch-all size class"""
    rng = np.random.default_rng(150)
    items = []
    while len(items) < 6:
        g, phases = common.gene_like_raw(rng, n_runs=520, strand="+-."[len(items) % 3])
        it = raw_item(g, phases, rng, 10000)
        if A.pre_assemble(it[0], phases, 10000)[3] == 0:
            items.append(it)
    with A.DecompBatch(0) as b:
        g_nv = add_all_raw(b, items)
        run(b)
        assert min(g_nv) > 1024
        used = {c for c in range(14) if b.class_info(c)["n_graphs"]}
        assert used and min(used) > 6, used
        got = b.features_all(None, raw_on_device=True)
        want = host_table(b, 6)
        assert assert_tables_equal(got, want) > 6
        res = b.result()                                              # the kernel's own bound: (offset, count) per path + two words per possible junction
        words = [2 * int(res.path_offset[g + 1] - res.path_offset[g]) +
                 2 * sum(max(int(res.pv_offset[p + 1] - res.pv_offset[p]) - 3, 0) for p in range(int(res.path_offset[g]), int(res.path_offset[g + 1]))) for g in range(6)]
        assert max(words) > 4096, words
        assert got["stats"]["host_graphs"] == 0


def test_invariant_graphs_empty_batch_and_reuse():
    rng = np.random.default_rng(8)
    with A.DecompBatch(0) as b:
        run(b)
        got = b.features_all(raw_on_device=True)                      # an empty batch
        assert got["rows"].size == 0 and got["graph_rc"].size == 0 and list(got["row_begin"]) == [0]
        # raw graphs that end with an invariant status: the pre-steps assert on a phase (no fold is involved), or an edge count is zero
        bad_items, _ = raw_draw(1079, 200, keep_asserted=True)
        assert len(bad_items) >= 5
        zero = []
        for it in raw_draw(1080, 40)[0]:
            it[0].edge_count[:] = 0
            zero.append(it)
        good, _ = raw_draw(1081, 40)
        items = bad_items + zero + good
        g_nv = add_all_raw(b, items); n = len(items)
        run(b)
        st = b.result().status
        ex = random_extras(g_nv, rng)
        first = b.features_all(ex, g_nv=g_nv, raw_on_device=True)
        inv = np.nonzero(st >= 100)[0]
        assert (st[:len(bad_items)] >= 100).all() and inv.size > len(bad_items)
        assert (np.diff(first["row_begin"])[inv] == 0).all() and (first["graph_rc"][inv] == 0).all()
        want = host_table(b, n, ex)
        # the host routine re-runs the pre-steps and so reports their assert once more for a graph that has no rows anyway; everything
        # else is equal
        assert (want[2][:len(bad_items)] != 0).all() and (want[2][len(bad_items):] == 0).all()
        rc = first["graph_rc"].copy(); rc[:len(bad_items)] = want[2][:len(bad_items)]
        assert assert_tables_equal(dict(first, graph_rc=rc), want) > 30
        assert first["stats"]["host_graphs"] == 0
        # reuse: a different, larger raw batch on the same object -- the overlay grows and its dead flags are not stale
        b.clear()
        more, folds = raw_draw(1082, 220)
        assert folds > 50 and sum(int(it[0].g_ne[0]) for it in more) > sum(int(it[0].g_ne[0]) for it in items)
        g_nv = add_all_raw(b, more)
        run(b)
        ex = random_extras(g_nv, rng)
        second = b.features_all(ex, g_nv=g_nv, raw_on_device=True)
        assert assert_tables_equal(second, host_table(b, len(more), ex)) > 300
        assert second["stats"]["host_graphs"] == 0 and second["stats"]["device_graphs"] == len(more)


def test_unknown_flag_bits_on_a_downloaded_batch():
    lib = A.load_library()
    with A.DecompBatch(0) as b:
        run(b)
        assert lib.ald_batch_features_all_ex(b._h, None, 2) == -1
        assert lib.ald_batch_features_all_ex(b._h, None, 0x80000001) == -1
        assert lib.ald_batch_features_all_ex(b._h, None, 1) == 0


def _adapter_input(items, extras):
    lines = ["%d" % len(items)]
    for (one, phases, dist), x in zip(items, extras):
        V, E = int(one.g_nv[0]), int(one.g_ne[0])
        lines.append("%d %d %d %d %d %d" % (V, E, len(phases), x["reads"], x["subgraph"], dist))
        for i in range(V):
            lines.append("%r %d %d %r %r %r %r %d %r %d %r" % (float(one.vertex_weight[i]), int(one.vertex_lpos[i]), int(one.vertex_rpos[i]),
                         *[float(x[k][i]) for k in ("l1", "l2", "l3", "lm")], int(x["lc"][i]), float(x["lr"][i]), int(x["cc"][i]), float(x["cr"][i])))
        src = np.repeat(np.arange(V), np.diff(one.vertex_offset))
        for k in np.argsort(one.edge_rank, kind="stable"):           # creation order
            lines.append("%d %d %r %d" % (int(src[k]), int(one.edge_target[k]), float(one.edge_weight[k]), int(one.edge_count[k])))
        for co, c in phases:
            lines.append("%d %d %s" % (len(co), c, " ".join(str(int(v)) for v in co)))
    return "\n".join(lines) + "\n"


def test_cpp_adapter_raw_on_device_gives_the_same_values():
    exe = os.path.join(ROOT, "tests", "_build", "features_raw_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "aletsch_amd", "lib")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_adapter", "features_raw_test.cc"), "-o", exe, "-L" + lib, "-laletsch_decomp", "-Wl,-rpath," + lib], check=True)
    items, folds = raw_draw(1083, 24)
    assert folds > 5
    rng = np.random.default_rng(9)
    raw = []
    for it in items:
        V = int(it[0].g_nv[0])
        raw.append(dict(reads=int(rng.integers(1, 500)), subgraph=int(rng.integers(0, 3)), l1=rng.random(V), l2=rng.random(V), l3=rng.random(V), lm=rng.random(V),
                        lc=rng.integers(0, 9, V), lr=rng.random(V), cc=rng.integers(0, 9, V), cr=rng.random(V)))
    r = subprocess.run([exe], input=_adapter_input(items, raw), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = r.stdout.splitlines()
    n = len(items)
    assert "round 0 device_graphs 0 host_graphs %d" % n in out and "round 1 device_graphs %d host_graphs 0" % n in out
    n_rows = sum(int(ln.split()[-1]) for ln in out if ln.startswith("graph "))
    assert n_rows > 40
