"""GPU tier: ald_batch_features_all -- the feature block of every transcript of a downloaded batch in one device pass (trst_features.hip) --
against the per-graph host routine ald_batch_features (the yardstick) row for row and field for field, bit for bit, with the same per-graph
return code; and against the oracle directly on the workload of test_gpu_parity.py::test_transcript_features_match_oracle."""
import os
import subprocess

import numpy as np
import pytest

import aletsch_amd as A
import common

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


def assert_tables_equal(got, want, check_asserted_rows=False):
    rows, comp, rc, rb = want
    assert np.array_equal(got["row_begin"], rb)
    assert np.array_equal(got["graph_rc"], rc), np.nonzero(got["graph_rc"] != rc)[0][:10]
    assert np.array_equal(got["complete"], comp)
    keep = np.ones(len(comp), bool)
    if not check_asserted_rows:                                      # the reference would have aborted there: partial values mean nothing
        for g in np.nonzero(rc != 0)[0]:
            keep[rb[g]:rb[g + 1]] = False
    for name in A.FEATURE_DTYPE.names:
        a, w = _bits(got["rows"], name)[keep], _bits(rows, name)[keep]
        assert np.array_equal(a, w), (name, np.nonzero(a != w)[0][:5])
    return int(keep.sum())


def random_extras(pg, rng):
    out = []
    for V in pg.g_nv:
        V = int(V)
        out.append(A.GraphExtras.from_arrays(gr_reads=int(rng.integers(1, 10000)), gr_subgraph=int(rng.integers(0, 4)),
                                             boundary_loss1=rng.random(V), boundary_loss2=rng.random(V), boundary_loss3=rng.random(V), boundary_merged_loss=rng.random(V),
                                             unbridge_leaving_count=rng.integers(0, 9, V), unbridge_leaving_ratio=rng.random(V),
                                             unbridge_coming_count=rng.integers(0, 9, V), unbridge_coming_ratio=rng.random(V)))
    return out


def oracle_workload():
    pg = A.synth(seed=52, n_graphs=300, v_min=8, v_max=70, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=3, n_samples=3)
    rng = np.random.default_rng(3)
    pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
    return pg, random_extras(pg, rng)


def test_oracle_workload_against_host_routine_and_oracle(monkeypatch):
    pg, extras = oracle_workload()
    _, want_o = common.oracle_features(pg, extras)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        got = b.features_all(extras, g_nv=pg.g_nv)
        want = host_table(b, pg.n, extras)
        n = assert_tables_equal(got, want)
        assert got["stats"]["device_graphs"] == pg.n and got["stats"]["host_graphs"] == 0 and got["stats"]["device_ms"] > 0
        # the same with the junction lists of every graph in the scratch instead of LDS
        monkeypatch.setenv("ALD_DEBUG_FEAT_LDS", "0")
        again = b.features_all(A.BatchExtras.from_graph_extras(extras, pg.g_nv))
        monkeypatch.delenv("ALD_DEBUG_FEAT_LDS")
        assert_tables_equal(again, want)
    # and the oracle's own restatement
    n_complete = n_single = n_assert = 0
    for g in range(pg.n):
        wf, wc, wbad = want_o[g]
        assert (got["graph_rc"][g] != 0) == wbad, g
        if wbad:
            n_assert += 1; continue
        r0 = got["row_begin"][g]
        assert np.array_equal(got["complete"][r0:r0 + len(wc)], wc), g
        for k in range(len(wc)):
            row = got["rows"][r0 + k]
            if wc[k]:
                d = {x: row[x].item() for x in A.FEATURE_DTYPE.names}
                assert d == wf[k], (g, k)
                n_complete += 1
            else:
                n_single += 1
    assert n > 500 and n_complete > 500 and n_single > 0, (n, n_complete, n_single, n_assert)


def test_cfg3_like_batch_reaches_large_classes_and_scratch(monkeypatch):
    pg = A.synth(seed=1003, n_graphs=1500, v_min=8, v_max=512, edges_per_vertex=4, layout_mode=1)
    big = A.synth(seed=1004, n_graphs=6, v_min=1500, v_max=3000, edges_per_vertex=3, layout_mode=1)
    from aletsch_amd.packed import PackedGraphs
    pg = PackedGraphs.concat([pg, big])
    rng = np.random.default_rng(11)
    extras = A.BatchExtras.from_arrays(boundary_loss1=rng.random(int(pg.g_nv.sum())), unbridge_coming_count=rng.integers(0, 5, int(pg.g_nv.sum())),
                                       gr_reads=rng.integers(0, 100, pg.n))
    per_graph = []
    off = np.concatenate([[0], np.cumsum(pg.g_nv)])
    for g in range(pg.n):
        per_graph.append(A.GraphExtras.from_arrays(gr_reads=int(extras.arrays["gr_reads"][g]), boundary_loss1=extras.arrays["boundary_loss1"][off[g]:off[g + 1]],
                                                   unbridge_coming_count=extras.arrays["unbridge_coming_count"][off[g]:off[g + 1]]))
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        used = {c for c in range(14) if b.class_info(c)["n_graphs"]}
        assert used & {9, 10, 11, 12, 13}, used
        got = b.features_all(extras)
        assert_tables_equal(got, host_table(b, pg.n, per_graph))
        assert got["rows"].size > 10000


def test_abandoned_capacity_attempts(monkeypatch):
    """graphs started too low (ALD_DEBUG_UNDERCLASS): the pool holds records of the abandoned attempts, which the index never names"""
    pg = A.synth(seed=78, n_graphs=300, v_min=20, v_max=300, edges_per_vertex=4, phasing_per_graph=3, layout_mode=1)
    monkeypatch.setenv("ALD_DEBUG_UNDERCLASS", "2")
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        monkeypatch.delenv("ALD_DEBUG_UNDERCLASS")
        assert_tables_equal(b.features_all(), host_table(b, pg.n))


def test_invariant_status_graphs_and_single_exon_paths():
    pg = A.synth(seed=91, n_graphs=400, v_min=6, v_max=60, edges_per_vertex=3, n_samples=3, phasing_per_graph=3, weight_mode=1, layout_mode=1)
    rng = np.random.default_rng(7)
    cnt = pg.sample_counts() + rng.integers(0, 4, pg.edge_target.size).astype(np.int32)
    cnt[rng.random(cnt.size) < 0.01] = 0
    pg.edge_count = cnt.astype(np.int32)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        st = b.result().status
        got = b.features_all(None)
        want = host_table(b, pg.n)
        assert_tables_equal(got, want)
    bad = np.nonzero(st >= 100)[0]
    assert bad.size > 0                                               # graphs that ended with an invariant status have no rows
    assert (got["row_begin"][bad + 1] == got["row_begin"][bad]).all() and (got["graph_rc"][bad] == 0).all()
    assert (got["complete"] == 0).any() and (got["complete"] == 1).any()
    single = got["rows"][got["complete"] == 0]
    assert (single["seq_min_wt"] == 0).all() and (single["num_vertices"] > 0).all()
    assert (got["rows"]["gr_reads"] == 0).all() and (got["rows"]["start_loss1"] == 0).all()     # extras = NULL


def test_parallel_edges():
    """staged graphs with parallel edges: edge(s, t) is the NEWEST of them (the last in the out-row); the in / out sums add every one"""
    from aletsch_amd.packed import PackedGraphs
    rng = np.random.default_rng(5)
    graphs = []
    for t in range(200):
        g, _ = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 10)), strand="+-."[t % 3])
        V = int(g["V"])
        dup = [e for e in g["edges"] if e[0] > 0 and e[1] < V - 1 and rng.random() < 0.2]
        g["edges"] = list(g["edges"]) + [(e[0], e[1], float(e[2]) * 0.5 + 1.0) + tuple(e[3:]) for e in dup]
        graphs.append(g)
    pp = PackedGraphs.from_graphs(graphs)
    with A.DecompBatch(0) as b:
        b.add(pp); b.upload(); b.run(); b.download()
        got = b.features_all()
        n = assert_tables_equal(got, host_table(b, pp.n))
    assert n > 100


def test_mixed_raw_and_staged_graphs():
    from aletsch_amd.packed import PackedGraphs
    rng = np.random.default_rng(1076)
    staged = A.synth(seed=33, n_graphs=60, v_min=8, v_max=60, edges_per_vertex=3, layout_mode=1, weight_mode=2)
    n_raw = 0
    order = []
    with A.DecompBatch(0) as b:
        for t in range(120):
            if t % 2 == 0:
                g, phases = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 10)), strand="+-."[t % 3])
                one = PackedGraphs.from_graphs([g])
                one.edge_count = (one.sample_counts() + rng.integers(0, 3, one.edge_target.size)).astype(np.int32)
                assert b.add_raw(one, phases, 10000) == 0
                n_raw += 1; order.append(int(one.g_nv[0]))
            else:
                one = staged.select(np.array([t // 2]))
                b.add(one); order.append(int(one.g_nv[0]))
        b.upload(); b.run(); b.download()
        ex = []
        for V in order:
            ex.append(A.GraphExtras.from_arrays(gr_reads=int(rng.integers(1, 99)), boundary_loss2=rng.random(V), unbridge_leaving_ratio=rng.random(V)))
        got = b.features_all(ex, g_nv=order)
        assert got["stats"]["host_graphs"] == n_raw and got["stats"]["device_graphs"] == 120 - n_raw
        assert_tables_equal(got, host_table(b, 120, ex))
        assert (got["graph_rc"][0::2] != 0).any() or got["rows"].size > 100


def test_empty_batch_clear_and_reuse():
    with A.DecompBatch(0) as b:
        with pytest.raises(A.DecompError) as e:                       # before a download there is no table
            b.features_all()
        assert e.value.code == -4
        b.upload(); b.run(); b.download()
        got = b.features_all()
        assert got["rows"].size == 0 and got["graph_rc"].size == 0 and list(got["row_begin"]) == [0]
        pg, extras = oracle_workload()
        b.add(pg.select(np.arange(100))); b.upload(); b.run(); b.download()
        first = b.features_all(extras[:100], g_nv=pg.g_nv[:100])
        assert_tables_equal(first, host_table(b, 100, extras[:100]))
        b.clear()
        with pytest.raises(A.DecompError) as e:                       # clear() drops the table
            b.features_table()
        assert e.value.code == -4
        b.add(pg.select(np.arange(100, 300))); b.upload(); b.run(); b.download()
        with pytest.raises(A.DecompError):                            # a new download too
            b.features_table()
        second = b.features_all(extras[100:], g_nv=pg.g_nv[100:])
        assert_tables_equal(second, host_table(b, 200, extras[100:]))


def _adapter_input(pg, extras):
    lines = ["%d" % pg.n]
    off = np.concatenate([[0], np.cumsum(pg.g_nv)])
    for g in range(pg.n):
        one = pg.select(np.array([g])); x = extras[g]
        V, E, P = int(one.g_nv[0]), int(one.g_ne[0]), int(one.g_np[0])
        lines.append("%d %d %d %d %d" % (V, E, P, x["reads"], x["subgraph"]))
        for i in range(V):
            lines.append("%r %d %d %r %r %r %r %d %r %d %r" % (float(one.vertex_weight[i]), int(one.vertex_lpos[i]), int(one.vertex_rpos[i]),
                         *[float(x[k][i]) for k in ("l1", "l2", "l3", "lm")], int(x["lc"][i]), float(x["lr"][i]), int(x["cc"][i]), float(x["cr"][i])))
        for s in range(V):
            for k in range(one.vertex_offset[s], one.vertex_offset[s + 1]):
                lines.append("%d %d %r %d" % (s, int(one.edge_target[k]), float(one.edge_weight[k]), int(one.edge_count[k])))
        for p in range(P):
            vs = one.phasing_vertex[one.phasing_offset[p]:one.phasing_offset[p + 1]]
            lines.append("%d %d %s" % (len(vs), int(one.phasing_count[p]), " ".join(str(int(v)) for v in vs)))
    return "\n".join(lines) + "\n"


def test_cpp_adapter_features_equal_the_table():
    exe = os.path.join(ROOT, "tests", "_build", "features_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "aletsch_amd", "lib")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_adapter", "features_test.cc"),
                    "-o", exe, "-L" + lib, "-laletsch_decomp", "-Wl,-rpath," + lib], check=True)
    pg = A.synth(seed=64, n_graphs=8, v_min=10, v_max=50, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=4)
    pg.sample_id[:] = 0; pg.sample_abd[:] = pg.edge_weight; pg.edge_abd[:] = pg.edge_weight      # the mock edge_info: one sample, abd = weight
    rng = np.random.default_rng(9)
    pg.edge_count = rng.integers(1, 5, pg.edge_target.size).astype(np.int32)
    raw = []
    for V in pg.g_nv:
        V = int(V)
        raw.append(dict(reads=int(rng.integers(1, 500)), subgraph=int(rng.integers(0, 3)), l1=rng.random(V), l2=rng.random(V), l3=rng.random(V), lm=rng.random(V),
                        lc=rng.integers(0, 9, V), lr=rng.random(V), cc=rng.integers(0, 9, V), cr=rng.random(V)))
    r = subprocess.run([exe], input=_adapter_input(pg, raw), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # the same graphs through the Python binding: even graphs with their extras, odd ones without
    ex = [A.GraphExtras.from_arrays(gr_reads=x["reads"], gr_subgraph=x["subgraph"], boundary_loss1=x["l1"], boundary_loss2=x["l2"], boundary_loss3=x["l3"],
                                    boundary_merged_loss=x["lm"], unbridge_leaving_count=x["lc"], unbridge_leaving_ratio=x["lr"],
                                    unbridge_coming_count=x["cc"], unbridge_coming_ratio=x["cr"]) if g % 2 == 0 else None for g, x in enumerate(raw)]
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        t = b.features_all(ex, g_nv=pg.g_nv)
    names = A.FEATURE_DTYPE.names
    want = []
    for rnd in range(2):
        for g in range(pg.n):
            r0, r1 = t["row_begin"][g], t["row_begin"][g + 1]
            want.append("round %d graph %d rc %d rows %d" % (rnd, g, t["graph_rc"][g], r1 - r0))
            for k in range(r0, r1):
                row = t["rows"][k]
                f = [str(int(t["complete"][k]))] + [("%016x" % int(np.float64(row[x]).view(np.uint64))) if A.FEATURE_DTYPE[x] == np.float64 else str(int(row[x])) for x in names]
                want.append(" ".join(f))
    assert r.stdout.splitlines() == want
    assert t["rows"].size > 20 and (t["complete"] == 1).any()
