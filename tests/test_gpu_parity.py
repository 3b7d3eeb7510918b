"""GPU parity tests proper: the HIP path (through the C ABI) against the oracle on the same seeded inputs.
Bit-exact: identical path sets in identical order, exact integer fields, bit-identical FP64 weight / abd / reads;
conf (exp of summed libm logs, reported only) within 1e-9 relative."""
import os

import numpy as np
import pytest

import aletsch_amd as A
import common
import device_run as DR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(common.PARITY_CONFIGS))
def test_hip_matches_oracle(name):
    pg = common.make_batch(name)
    want = common.oracle_run(pg)[0]
    got = A.decompose(pg, device=0)
    bad = common.compare_results(want, got, pg.n, conf_tol=1e-9)
    assert not bad, f"{name}: {len(bad)} mismatches, first {bad[:3]}"
    assert int((got.status != 0).sum()) == 0


def test_iteration_counts_match_oracle():
    pg = A.synth(**common.PARITY_CONFIGS["cfg2_64v256e"])
    want, st, _, _ = common.oracle_run(pg)
    assert not DR.oracle_mismatches("cfg2_64v256e", DR.run(pg), want, st[:, 3])


def test_op_trace_matches_oracle_on_gpu():
    pg = A.synth(**dict(common.PARITY_CONFIGS["everything"], n_graphs=40))
    want, st, _, traces = common.oracle_run(pg, trace=True)
    assert not DR.oracle_mismatches("everything", DR.run(pg, trace_cap=4096), want, st[:, 3], traces)


def test_nondefault_parameters_on_gpu():
    p = A.default_params()
    p.max_decompose_error_ratio[7] = 1.5; p.max_decompose_error_ratio[0] = 0.2; p.min_transcript_coverage = 5.0
    pg = A.synth(seed=31, n_graphs=200, v_min=10, v_max=70, edges_per_vertex=3, phasing_per_graph=8, weight_mode=1)
    want = common.oracle_run(pg, params=p)[0]
    got = A.decompose(pg, 0, p)
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)


def test_edge_cases_on_gpu():
    from aletsch_amd.packed import PackedGraphs
    graphs = [
        dict(V=2, edges=[], vw=[0, 0], lpos=[0, 0], rpos=[0, 0]),
        dict(V=4, edges=[(0, 1, 5.0), (1, 2, 5.0), (2, 3, 5.0)], vw=[0, 10, 10, 0], lpos=[0, 100, 300, 400], rpos=[0, 200, 400, 400]),
        dict(V=4, edges=[(0, 1, 1.0), (1, 3, 1.0)], vw=[0, 1, 1, 0], lpos=[0, 100, 300, 400], rpos=[0, 200, 400, 400]),
        dict(V=5, edges=[(0, 1, 9.0), (1, 2, 4.0), (1, 3, 5.0), (3, 4, 5.0)], vw=[0, 3, 3, 3, 0], lpos=[0, 10, 30, 50, 60], rpos=[0, 20, 40, 60, 60]),
        dict(V=4, edges=[(0, 1, 5.0, 0, {}), (1, 2, 5.0), (2, 3, 5.0)], vw=[0, 10, 10, 0], lpos=[0, 100, 300, 400], rpos=[0, 200, 400, 400]),
        dict(V=5, edges=[(0, 1, 6.0, 0, {1: 6.0}), (1, 2, 6.0, 0, {2: 6.0}), (2, 3, 6.0, 0, {1: 6.0}), (3, 4, 6.0, 0, {1: 6.0})], vw=[0, 1, 1, 1, 0], lpos=[0, 10, 30, 50, 60], rpos=[0, 20, 40, 60, 60]),
        dict(V=4, edges=[(0, 1, 5.0), (1, 2, 5.0), (2, 3, 5.0)], vw=[0, 10, 10, 0], lpos=[0, 100, 300, 400], rpos=[0, 200, 400, 400], vtype=[-1, -9, -1, -1]),
        dict(V=6, edges=[(0, 1, 8.0, 1), (0, 2, 6.0, 2), (1, 3, 8.0, 1), (2, 3, 6.0, 2), (3, 4, 7.0, 1), (3, 5, 7.0, 2), (4, 5, 7.0, 1)], vw=[0, 1, 1, 1, 1, 0],
             lpos=[0, 10, 30, 50, 70, 80], rpos=[0, 20, 40, 60, 80, 80]),
    ]
    pg = PackedGraphs.from_graphs(graphs)
    want = common.oracle_run(pg)[0]
    got = A.decompose(pg, 0)
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)
    # an empty batch is legal
    with A.DecompBatch(0) as b:
        b.upload(); b.run(); b.download()
        assert len(b.result().status) == 0


def test_subsetsum_kernel_matches_reference_golden():
    """HIP subset-sum DP against the answers of the reference's own subsetsum.cc (tests/golden/ref_subsetsum.json),
    first instance = the reference's KAT (subsetsum.cc:263-282)"""
    import json, os
    d = json.load(open(os.path.join(common.ROOT, "tests", "golden", "ref_subsetsum.json")))
    inst = [([tuple(x) for x in i["s"]], [tuple(x) for x in i["t"]]) for i in d["instances"]]
    got = A.subsetsum_batch(inst, 0)
    for g, ans in zip(got, d["answers"]):
        if ans is None:
            assert g is None
        else:
            assert g is not None and g[0] == ans["e"] and g[1] == ans["s"] and g[2] == ans["t"]
    assert got[0][1] == [3, 1] and got[0][2] == [2]


def test_full_size_properties():
    """BASELINE configs[1] at full size (100k x 64v/256e): size-independent properties of the decomposition"""
    n = 100000
    pg = A.synth(seed=1002, n_graphs=n, v_min=64, v_max=64, fixed_edges=256)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        r1 = b.result(); raw1 = b.raw_records()
        b.run(); b.download()
        r2 = b.result()
    assert (r1.status == 0).all()
    # idempotent / deterministic: a second run of the same resident batch gives the same answer
    assert not common.compare_results(r1, r2, n)
    # every path runs source -> sink along edges of the ORIGINAL graph, vertices strictly ascending
    src = np.repeat(np.tile(np.arange(64), n), np.diff(pg.vertex_offset.reshape(n, 65), axis=1).reshape(-1))
    key = (np.repeat(np.arange(n, dtype=np.int64), 256) * 64 + src) * 64 + pg.edge_target
    keys = np.sort(key)
    gid = np.repeat(np.arange(n, dtype=np.int64), np.diff(r1.path_offset))
    pv = r1.path_vertices.astype(np.int64); po = r1.pv_offset
    first = pv[po[:-1]]; last = pv[po[1:] - 1]
    assert (first == 0).all() and (last == 63).all()
    a = np.delete(pv, po[1:] - 1); bnext = np.delete(pv, po[:-1])                # consecutive pairs inside each path
    pg_of_pair = np.repeat(gid, np.diff(po) - 1)
    assert (bnext > a).all()
    k = (pg_of_pair * 64 + a) * 64 + bnext
    idx = np.searchsorted(keys, k)
    assert (keys[np.minimum(idx, len(keys) - 1)] == k).all()
    # weights are positive, above the reporting threshold only for greedy paths; lengths = 200 * internal vertices
    assert (r1.weight > 0).all()
    assert np.array_equal(r1.length, 200 * (np.diff(po) - 2))
    # sharding invariance: the first 1000 graphs decomposed alone give the same paths (graphs are independent)
    sub = A.decompose(pg.select(np.arange(1000)), 0)
    lim = int(r1.path_offset[1000])
    assert np.array_equal(sub.path_offset, r1.path_offset[:1001]) and np.array_equal(sub.weight, r1.weight[:lim])
    assert np.array_equal(sub.path_vertices, r1.path_vertices[: int(r1.pv_offset[lim])])
    # oracle parity on the WHOLE full-size batch (the oracle runs on all host cores: ~10 s); rare interleavings of the rule cascade
    # only show up at this scale (a stale evaluation that changed 7 graphs in 100 000 was caught exactly here)
    want = common.oracle_run(pg, threads=DR.THREADS)[0]
    assert not common.compare_results(want, r1, n, conf_tol=1e-9)


def test_transcripts_match_oracle():
    """exon join + coverage = log(1 + weight) (scallop.cc:3250-3266, essential.cc:719-748) against the oracle's build_transcripts;
    layout_mode=1 makes ~30% of consecutive vertices touch, so joins do happen"""
    pg = A.synth(seed=44, n_graphs=120, v_min=8, v_max=80, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=4)
    _, cov_o, eo_o, lr_o = common.oracle_transcripts(pg)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        cov, eo, lr = b.transcripts()
        r = b.result()
    assert np.array_equal(eo, eo_o) and np.array_equal(lr, lr_o)
    assert np.array_equal(cov, cov_o)                       # host libm on both sides, bit-identical weights
    assert (np.diff(eo) < np.diff(r.pv_offset) - 2).any()   # at least one path had touching exons joined


def test_batch_into_result_sink():
    """ald_tset_add_batch (graph by graph, assembler.cc:1105-1133) == feeding the exported transcripts through ald_tset_add,
    whose merge rules are pinned to the reference's transcript_set.cc by tests/test_tset_cpu.py"""
    pg = A.synth(seed=45, n_graphs=200, v_min=8, v_max=40, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2)
    sid = (np.arange(pg.n) % 5).astype(np.int32)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        cov, eo, lr = b.transcripts(); r = b.result()
        s = A.TranscriptSink(0.8); s.add_batch(b, sid, tid_base=0)
    groups = []
    for g in range(pg.n):
        ts = []
        for k, i in enumerate(range(r.path_offset[g], r.path_offset[g + 1])):
            ts.append((chr(r.strand[i]), float(cov[i]), float(r.conf[i]), float(r.abd[i]), int(r.count[i]), (g << 20) | k, [tuple(map(int, e)) for e in lr[eo[i]:eo[i + 1]]]))
        groups.append((int(sid[g]), ts))
    t = A.TranscriptSink(0.8); t.add_groups(groups)
    a, c = s.items(), t.items()
    assert len(a) > 0 and a == c
    assert sum(x["count"] for x in a) == len(cov)           # every transcript landed in exactly one item
    # the batch merge deals the hash buckets to host threads: any number of threads, and a sink that already holds items, give the same set
    import os
    for thr in ("1", "3", "8"):
        os.environ["ALD_SINK_THREADS"] = thr
        try:
            with A.DecompBatch(0) as b:
                b.add(pg); b.upload(); b.run(); b.download()
                u = A.TranscriptSink(0.8); u.add_batch(b, sid, tid_base=0)
                w = A.TranscriptSink(0.8); w.add_batch(b, sid, tid_base=0); w.add_batch(b, (sid + 1) % 5, tid_base=1 << 40)
        finally:
            del os.environ["ALD_SINK_THREADS"]
        assert u.items() == a
        if thr == "1":
            twice = w.items()
        else:
            assert w.items() == twice


def test_large_classes_on_gpu():
    """V > 512: class 9 (one workgroup per CU, 145 KB of LDS) up to 1024 vertices, beyond that the catch-all class 10 with its hot
    state in HBM; mixed with small graphs in the same batch (concurrent class streams)"""
    big = A.synth(seed=99, n_graphs=3, v_min=900, v_max=1000, edges_per_vertex=4)
    huge = A.synth(seed=97, n_graphs=2, v_min=1200, v_max=1500, edges_per_vertex=3)
    small = A.synth(seed=98, n_graphs=40, v_min=8, v_max=120, edges_per_vertex=3)
    from aletsch_amd.packed import PackedGraphs
    pg = PackedGraphs.concat([small, big, huge])
    want = common.oracle_run(pg)[0]
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        got = b.result()
        assert b.class_info(9)["n_graphs"] == 3 and b.class_info(10)["n_graphs"] == 2
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)


def test_class_beyond_the_catch_all_on_gpu():
    """2 500-vertex graphs run in the largest class (class 13: hot state in the slab, 32-bit creation ids) and match the oracle; a graph
    beyond every class is refused with ALD_ST_TOO_LARGE, the rest of its batch is unaffected"""
    pg = A.synth(seed=78, n_graphs=3, v_min=2500, v_max=2500, edges_per_vertex=3)
    want = common.oracle_run(pg, threads=3)[0]
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download(); got = b.result()
        assert b.class_info(13)["n_graphs"] == 3
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)
    small = A.synth(seed=79, n_graphs=50, v_min=10, v_max=60, edges_per_vertex=3)
    huge = A.synth(seed=5, n_graphs=1, v_min=10300, v_max=10300, edges_per_vertex=2)
    want = common.oracle_run(small, threads=4)[0]
    with A.DecompBatch(0) as b:
        b.add(small); b.add(huge); b.upload(); b.run(); b.download(); got = b.result()
        gf = b.result_index()[1]
    assert got.status[50] == 4 and np.diff(got.path_offset)[50] == 0
    assert gf[50] == -1 and (gf[:50][np.diff(got.path_offset)[:50] > 0] >= 0).all()      # a graph no wave ever ran: "no records" in the result index, not stale memory
    import dataclasses
    first = dataclasses.replace(got, status=got.status[:50], path_offset=got.path_offset[:51])       # (the refused graph has no paths)
    assert not common.compare_results(want, first, small.n, conf_tol=1e-9)


def test_max_num_exons_on_gpu():
    """|V| > max_num_exons: cascade skipped, greedy phase only (scallop.cc:49), status ALD_ST_SKIPPED_LARGE"""
    p = A.default_params(); p.max_num_exons = 30
    pg = A.synth(seed=55, n_graphs=400, v_min=10, v_max=120, edges_per_vertex=3, weight_mode=2, phasing_per_graph=2)
    want = common.oracle_run(pg, params=p, threads=4)[0]
    got = A.decompose(pg, device=0, params=p)
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)
    assert (got.status[pg.g_nv > 30] == 1).all() and (got.status[pg.g_nv <= 30] == 0).any()


def test_capacity_retry_on_gpu():
    """graphs started two classes too low (ALD_DEBUG_UNDERCLASS): CAPACITY -> re-queued one class up inside ald_batch_download until
    they fit; same answer; and a second run of the same resident batch (first pass re-staged after the retries) as well"""
    import os
    pg = A.synth(seed=78, n_graphs=300, v_min=20, v_max=300, edges_per_vertex=4, phasing_per_graph=3)
    want = common.oracle_run(pg, threads=4)[0]
    os.environ["ALD_DEBUG_UNDERCLASS"] = "2"
    try:
        with A.DecompBatch(0) as b:
            b.add(pg); b.upload()
            import ctypes as C
            for rep in range(2):
                b.run()
                # the retry passes of the previous download regrew class slabs (hipFree + hipMalloc): the first pass of this run must
                # have been launched with the buffers the batch owns NOW, not the addresses staged at upload time
                for c in range(14):
                    if b.class_info(c)["blocks_last_run"] > 0:
                        used, owned = C.c_void_p(), C.c_void_p()
                        assert b._lib.ald_batch_debug_slab(b._h, c, C.byref(used), C.byref(owned)) == 0
                        assert used.value == owned.value, (rep, c)
                b.download()
                assert not common.compare_results(want, b.result(), pg.n, conf_tol=1e-9)
    finally:
        del os.environ["ALD_DEBUG_UNDERCLASS"]


def test_explicit_edge_counts_on_gpu():
    """edge_info.count handed over separately from the sample sets (see tests/test_emu_vs_oracle.py)"""
    pg = A.synth(seed=91, n_graphs=300, v_min=8, v_max=90, edges_per_vertex=3, n_samples=3, phasing_per_graph=3, weight_mode=1)
    rng = np.random.default_rng(7)
    cnt = pg.sample_counts() + rng.integers(0, 4, pg.edge_target.size).astype(np.int32)
    cnt[rng.random(cnt.size) < 0.002] = 0
    pg.edge_count = cnt.astype(np.int32)
    want = common.oracle_run(pg)[0]
    got = A.decompose(pg, device=0)
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)


def test_record_exchange_from_device_memory():
    """the multi-GPU exchange step with one rank over RCCL: the record pool is handed over in HBM (zero-copy view of
    ald_batch_device_records) and comes back on rank 0 identical to the host copy, graph ids made global by the C helper"""
    import os
    import torch
    import torch.distributed as dist
    from aletsch_amd.distributed import RecordGatherer, _device_words, parse_records
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29541")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        pg = A.synth(seed=46, n_graphs=500, v_min=8, v_max=60, edges_per_vertex=3)
        with A.DecompBatch(0) as b:
            b.add(pg); b.upload(); b.run(); b.download()
            raw = b.raw_records(); ptr, n = b.device_records()
            assert n == raw.size and ptr != 0
            g = RecordGatherer(torch.device("cuda", 0))
            for rep in range(2):                                   # buffers are reused on the second step
                g.gather(_device_words(ptr, n, torch.device("cuda", 0)), graph_offset=1000)
                (words, off), = g.streams()
                assert off == 1000 and np.array_equal(words, raw)
            glob = A.records_add_graph_offset(words.copy(), off)
            recs = parse_records(glob); local = parse_records(raw)
            assert [r["graph"] for r in recs] == [r["graph"] + 1000 for r in local] and [r["v"] for r in recs] == [r["v"] for r in local]
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_rejected_graphs_leave_the_batch_intact():
    """Error behaviour of the staging calls: a malformed graph is refused with ALD_ERR_INVALID and a message, and the batch stays
    exactly as it was -- also when the defect is only found after part of the graph (or earlier graphs of the same bulk call) had
    been appended.  The graphs staged before and after the refused calls decompose as if nothing had happened."""
    import copy
    from aletsch_amd.native import DecompError
    pg = A.synth(seed=77, n_graphs=24, v_min=10, v_max=40, edges_per_vertex=3, n_samples=3, phasing_per_graph=4, weight_mode=1)
    want = common.oracle_run(pg)[0]
    first, second = pg.select(np.arange(0, 12)), pg.select(np.arange(12, 24))

    def broken(kind):
        bad = copy.deepcopy(pg.select(np.arange(3, 6)))           # three graphs in one bulk call; the defect sits in the LAST one
        sl = bad.graph_slices(); g = 2
        e0 = int(sl["e"][g]); vo0 = int(sl["vo"][g]); V = int(bad.g_nv[g])
        row = next(s for s in range(V) if bad.vertex_offset[vo0 + s + 1] - bad.vertex_offset[vo0 + s] >= 2)
        k = e0 + int(bad.vertex_offset[vo0 + row])
        if kind == "backward edge":
            s = next(s for s in range(2, V) if bad.vertex_offset[vo0 + s + 1] > bad.vertex_offset[vo0 + s])
            bad.edge_target[e0 + int(bad.vertex_offset[vo0 + s])] = s - 1
        elif kind == "self loop":
            bad.edge_target[k] = row
        elif kind == "strand out of range":
            bad.edge_strand[k + 1] = 3
        elif kind == "strand out of range, unsorted row":          # the element-wise path appends edges before it meets the defect
            bad.edge_target[k], bad.edge_target[k + 1] = bad.edge_target[k + 1], bad.edge_target[k]
            bad.edge_strand[k + 1] = 3
        elif kind == "negative edge count":
            bad.edge_count = bad.sample_counts().astype(np.int32); bad.edge_count[k] = -1
        elif kind == "vertex_offset does not span":
            bad.vertex_offset[vo0 + V] += 1
        elif kind == "two vertices at least":
            bad.g_nv[g] = 1
        return bad

    with A.DecompBatch(0) as b:
        b.add(first)
        for kind in ("backward edge", "self loop", "strand out of range", "strand out of range, unsorted row", "negative edge count",
                     "vertex_offset does not span", "two vertices at least"):
            with pytest.raises(DecompError) as ei:
                b.add(broken(kind))
            assert ei.value.code == -1, (kind, ei.value)                       # ALD_ERR_INVALID
            assert b.n == first.n, kind
        b.add(second)
        assert b.n == pg.n
        b.upload(); b.run(); b.download()
        got = b.result()
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)


@pytest.mark.gpu
def test_calls_out_of_order_are_refused():
    """run before upload, download before run, results before download: ALD_ERR_STATE with a message, never a crash or stale data;
    staging another graph invalidates what was uploaded."""
    from aletsch_amd.native import DecompError
    pg = A.synth(seed=78, n_graphs=8, v_min=8, v_max=20, edges_per_vertex=3)
    with A.DecompBatch(0) as b:
        b.add(pg)
        for call in (b.run, b.download, b.result):
            with pytest.raises(DecompError) as ei:
                call()
            assert ei.value.code == -4, ei.value                               # ALD_ERR_STATE
        b.upload()
        with pytest.raises(DecompError):
            b.download()
        b.add(pg.select(np.arange(2)))                                         # the wire buffer on the device is stale now
        with pytest.raises(DecompError):
            b.run()
        b.upload(); b.run(); b.download()
        assert (b.result().status == 0).all() and b.n == 10


@pytest.mark.gpu
def test_slab_twins_of_the_large_lds_classes(monkeypatch):
    """Classes 11 / 12 are the twins of 7 / 8 with the hot state in the wave's HBM slab (chosen when a batch holds more graphs of the
    class than its LDS form runs at once).  Forced on and forced off, the records are the same and equal the oracle's; a graph that
    outgrows a twin is retried through twin 12 and then class 9."""
    pg = A.synth(seed=93, n_graphs=60, v_min=390, v_max=512, edges_per_vertex=4, phasing_per_graph=6, n_samples=2, weight_mode=1)
    want = common.oracle_run(pg, threads=8)[0]
    for force in ("1", "0"):
        monkeypatch.setenv("ALD_DEBUG_TWIN", force)
        assert not DR.oracle_mismatches("twins " + force, DR.run(pg), want, want_classes={11, 12, 9} if force == "1" else {7, 8, 9})
    monkeypatch.setenv("ALD_DEBUG_TWIN", "1"); monkeypatch.setenv("ALD_DEBUG_UNDERCLASS", "1")
    small = pg.select(np.arange(12))
    with A.DecompBatch(0) as b:                               # started one class too low: overflow -> the next twin / class 9
        b.add(small); b.upload(); b.run(); b.download()
        got = b.result()
    w2 = common.oracle_run(small, threads=8)[0]
    assert not common.compare_results(w2, got, small.n, conf_tol=1e-9)


def test_cfg3_mixed_batch_at_spec():
    """BASELINE.json configs[2] at spec: 10 000 graphs, V ~ U{8..512}, E = 4V (seed 1003) -- the one place where nine
    size classes, three side streams and the LDS / slab-twin choice run together -- compared with the oracle graph by graph"""
    pg = A.synth(seed=1003, n_graphs=10000, v_min=8, v_max=512, edges_per_vertex=4)
    want = common.oracle_run(pg, threads=DR.THREADS)[0]
    r = DR.run(pg)
    assert not DR.oracle_mismatches("cfg3", r, want)
    assert (r.result.status == 0).all() and len(r.classes) >= 8, r.classes


def test_flow_weights_at_full_size():
    """SURVEY.md 8d's second weight distribution at the bench size: 100 000 x 64v/256e with flow-conserving weights (sums of random s-t
    paths); twice the unsplittable vertices and router runs of the uniform batch, and at least one graph outgrows its class and is
    retried one class up"""
    n = 100000
    pg = A.synth(seed=1002, n_graphs=n, v_min=64, v_max=64, fixed_edges=256, weight_mode=2)
    want = common.oracle_run(pg, threads=DR.THREADS)[0]
    r = DR.run(pg)
    assert not DR.oracle_mismatches("flow weights", r, want)
    assert (r.result.status == 0).all()
    assert set(r.classes) - {1}, f"expected at least one capacity retry out of class 1: {r.classes}"


def test_fuzz_slice():
    """A fixed-seed slice of the randomized GPU-vs-oracle sweep (60 s; profiles/r01/fuzz_parity.txt holds the long runs): sizes 4..520,
    2..5 edges per vertex, three weight modes, 1..4 samples, 0..25 phasing paths, strands, touching exons, non-default ratios,
    coverage threshold and max_num_exons, explicit edge counts, permuted creation ranks"""
    import time
    rng = np.random.default_rng(20260)
    thr = DR.THREADS
    t_end = time.time() + 60.0; ntot = 0; k = 0
    while time.time() < t_end:
        k += 1
        vmin = int(rng.choice([4, 8, 16, 32, 64, 100])); vmax = int(min(520, vmin * rng.choice([1, 2, 4])))
        kw = dict(seed=int(rng.integers(1, 1 << 30)), v_min=vmin, v_max=vmax, edges_per_vertex=int(rng.choice([2, 3, 4, 5])),
                  weight_mode=int(rng.choice([0, 1, 2])), n_samples=int(rng.choice([1, 1, 2, 4])), phasing_per_graph=int(rng.choice([0, 0, 3, 10, 25])),
                  strand_mode=int(rng.choice([0, 0, 1])), layout_mode=int(rng.choice([0, 1])))
        kw["n_graphs"] = int(max(50, min(20000, 2.5e6 / ((vmin + vmax) / 2 * kw["edges_per_vertex"]))))
        p = A.default_params()
        if rng.random() < 0.3: p.max_decompose_error_ratio[7] = float(rng.choice([1.2, 1.5, 3.0]))
        if rng.random() < 0.3: p.max_decompose_error_ratio[0] = float(rng.choice([0.1, 0.2, 0.5]))
        if rng.random() < 0.2: p.min_transcript_coverage = float(rng.choice([0.5, 5.0]))
        if rng.random() < 0.2: p.max_num_exons = int(rng.choice([12, 40, 150]))
        pg = A.synth(**kw)
        if rng.random() < 0.3:
            pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
        if rng.random() < 0.3:
            r = np.empty(pg.edge_target.size, np.int32); o = 0
            for e in pg.g_ne:
                r[o:o + e] = rng.permutation(int(e)); o += int(e)
            pg.edge_rank = r
        want = common.oracle_run(pg, params=p, threads=thr)[0]
        got = A.decompose(pg, device=0, params=p)
        bad = common.compare_results(want, got, pg.n, conf_tol=1e-9)
        assert not bad, (k, kw, list(p.max_decompose_error_ratio), p.min_transcript_coverage, p.max_num_exons, bad[:3])
        ntot += pg.n
    assert k >= 3 and ntot >= 1000, (k, ntot)


def test_edge_creation_rank_on_gpu():
    """the caller's edge order (position in gr.edges()) as the kernel's initial edge ids: permuted ranks change router / pe2w outcomes
    identically in HIP and oracle; the identity rank is the default"""
    import copy
    pg = A.synth(seed=21, n_graphs=2000, v_min=10, v_max=140, edges_per_vertex=3, phasing_per_graph=10, weight_mode=1, n_samples=3)
    base = A.decompose(pg, 0)
    ident = copy.copy(pg); ident.edge_rank = pg.identity_rank()
    assert not common.compare_results(base, A.decompose(ident, 0), pg.n)
    perm = copy.copy(pg); r = np.empty(pg.edge_target.size, np.int32); o = 0; rng = np.random.default_rng(8)
    for e in pg.g_ne:
        r[o:o + e] = rng.permutation(int(e)); o += int(e)
    perm.edge_rank = r
    want = common.oracle_run(perm, threads=DR.THREADS)[0]
    got = A.decompose(perm, 0)
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)
    assert common.compare_results(base, got, pg.n), "a permuted creation rank should change some decomposition"
    # a rank that is not a permutation is refused, the batch stays usable
    from aletsch_amd.native import DecompError
    bad = copy.copy(pg.select(np.arange(4))); bad.edge_rank = bad.identity_rank(); bad.edge_rank[1] = bad.edge_rank[0]
    with A.DecompBatch(0) as b:
        with pytest.raises(DecompError):
            b.add(bad)
        assert b.n == 0


def test_record_pool_regrow_on_gpu(monkeypatch):
    """a record pool that is too small: ALD_ST_POOL_FULL -> the pool grows, the batch runs again (no walk through the larger classes);
    a second run of the same resident batch uses the grown pool"""
    pg = A.synth(seed=33, n_graphs=600, v_min=20, v_max=90, edges_per_vertex=4)
    want = common.oracle_run(pg, threads=4)[0]
    plain = {}
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        plain = {c: b.class_info(c)["n_graphs"] for c in range(14)}
    monkeypatch.setenv("ALD_DEBUG_POOL_WORDS", "5000")
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload()
        for rep in range(2):
            b.run(); b.download()
            assert not common.compare_results(want, b.result(), pg.n, conf_tol=1e-9)
            assert {c: b.class_info(c)["n_graphs"] for c in range(14)} == plain


def test_transcript_stream_and_its_merge():
    """ald_batch_transcript_stream: the finished transcripts of a batch as one self-contained stream (what ranks exchange) --
    word for word the test-side restatement over the exported results; merging it (ald_tset_add_stream) gives the same set as
    ald_tset_add_batch, also when the batch is cut into two "ranks" whose streams are merged with their graph offsets"""
    pg = A.synth(seed=45, n_graphs=400, v_min=8, v_max=60, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)
    sid = (np.arange(pg.n) % 5).astype(np.int32)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        r = b.result()
        for skip in (False, True):
            w = b.transcript_stream(sid, skip_single_exon=skip)
            assert np.array_equal(w, common.transcript_stream_from_result(pg, r, sid, skip_single_exon=skip))
        w = b.transcript_stream(sid)
        direct = A.TranscriptSink(0.8); direct.add_batch(b, sid, tid_base=7 << 44)
    via = A.TranscriptSink(0.8); via.add_stream(w, tid_base=7 << 44)
    assert via.items() == direct.items() and len(via.items()) > 100
    cut = 170
    parts = []
    for lo, hi in ((0, cut), (cut, pg.n)):
        with A.DecompBatch(0) as b:
            b.add(pg.select(np.arange(lo, hi))); b.upload(); b.run(); b.download()
            parts.append((b.transcript_stream(sid[lo:hi]), lo))
    from aletsch_amd.distributed import merge_streams
    two = merge_streams(A.TranscriptSink(0.8), parts, tid_base=7 << 44)
    assert two.items() == direct.items()


def test_transcript_features_match_oracle():
    """ald_batch_features = scallop::update_trst_features + unique_junc (scallop.cc:3268-3497) read from the staged (original) graph:
    every one of the 41 fields of every transcript equals the oracle's container-based restatement bit for bit; single-exon paths are
    flagged incomplete on both sides; where the reference would have asserted (an intron of another path inside an exon whose
    flanking within-exon edges do not exist) both sides say so.  layout_mode=1 makes consecutive vertices touch, so exons span
    several vertices and retained introns do occur."""
    pg = A.synth(seed=52, n_graphs=300, v_min=8, v_max=70, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=3, n_samples=3)
    rng = np.random.default_rng(3)
    pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
    extras = []
    for V in pg.g_nv:
        V = int(V)
        extras.append(A.GraphExtras.from_arrays(gr_reads=int(rng.integers(1, 10000)), gr_subgraph=int(rng.integers(0, 4)),
                                                boundary_loss1=rng.random(V), boundary_loss2=rng.random(V), boundary_loss3=rng.random(V), boundary_merged_loss=rng.random(V),
                                                unbridge_leaving_count=rng.integers(0, 9, V), unbridge_leaving_ratio=rng.random(V),
                                                unbridge_coming_count=rng.integers(0, 9, V), unbridge_coming_ratio=rng.random(V)))
    want_r, want = common.oracle_features(pg, extras)
    n_complete = n_single = n_assert = n_intron = 0
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        assert not common.compare_results(want_r, b.result(), pg.n, conf_tol=1e-9)
        for g in range(pg.n):
            feats, comp, rc = b.features(g, extras[g])
            wf, wc, wbad = want[g]
            assert (rc != 0) == wbad, (g, rc, wbad)
            if wbad:
                n_assert += 1; continue                     # the reference would have aborted here: partial values mean nothing
            assert np.array_equal(comp, wc), g
            for k, f in enumerate(feats):
                d = f.as_dict()
                if comp[k]:
                    assert d == wf[k], (g, k, {x: (d[x], wf[k][x]) for x in d if d[x] != wf[k][x]})
                    n_complete += 1; n_intron += int(d["introns"] + d["start_introns"] + d["end_introns"] > 0)
                else:                                        # no junction: only the graph / path counts are defined
                    for x in ("gr_vertices", "gr_edges", "gr_reads", "gr_subgraph", "num_vertices", "num_edges", "max_mid_exon_len"):
                        assert d[x] == wf[k][x]
                    n_single += 1
        # without extras the boundary / unbridged fields read as zero
        f0, _, _ = b.features(0)
        assert all(f.start_loss1 == 0 and f.gr_reads == 0 for f in f0)
    assert n_complete > 500 and n_single > 0 and n_intron > 0, (n_complete, n_single, n_assert, n_intron)


def test_replayed_dumps_on_gpu():
    """graphs that arrive as the reference's text dump (splice_graph::write + hyper_set::write; aletsch_amd/graphio.py): parsed, staged
    with the creation order of the dump's lines, decomposed by the HIP kernels, compared with the oracle"""
    from aletsch_amd import graphio
    src = A.synth(seed=83, n_graphs=400, v_min=6, v_max=90, edges_per_vertex=3, weight_mode=1, phasing_per_graph=10, layout_mode=0)
    src.edge_strand[:] = 0; src.vertex_weight[:] = np.round(src.vertex_weight)
    pg, meta = graphio.read_bundle_dump(graphio.write_bundle_dump(src))
    assert pg.n == src.n and np.array_equal(pg.edge_weight, src.edge_weight)
    want = common.oracle_run(pg, threads=4)[0]
    got = A.decompose(pg, 0)
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)
    assert (got.status == 0).all()


def test_raw_graphs_through_the_pre_steps_on_gpu():
    """ald_batch_add_graph_raw: graphs as assembler::assemble(gx, px, sid) receives them + phase sets in exon
    coordinates go to the device as they are; the wave that loads a graph runs extend_strands / boundary grouping / phase projection /
    hyper_set ctor / filter_nodes (decomp_device.h: pre_assemble_device), then decomposes it.  Against the oracle's pre-steps +
    decomposition, graph for graph; where the reference would have asserted in the pre-steps the graph ends with an invariant status.
    The bulk entry point (ald_batch_add_packed_raw) must give the same batch, and the features of a raw graph must be read from the
    graph as scallop would have received it (gr_ori = the grouped graph)."""
    import ctypes as C
    from aletsch_amd.packed import PackedGraphs
    O = common.oracle_lib()
    O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]; O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
    rng = np.random.default_rng(1076)
    want_parts = []; asserted = []; raws = []; all_phases = []
    with A.DecompBatch(0) as b:
        for t in range(300):
            g, phases = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 10)), strand="+-."[t % 3])
            if t % 9 == 0:
                phases = phases + phases[:2]
            pg = PackedGraphs.from_graphs([g])
            pg.edge_rank = np.array(sorted(range(len(g["edges"])), key=lambda k: (g["edges"][k][0], g["edges"][k][1])), np.int32)
            pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
            want, _, _, rc_o = A.pre_assemble(pg, phases, 10000, _lib=O, _prefix="ora")
            assert b.add_raw(pg, phases, 10000) == 0
            asserted.append(rc_o != 0); raws.append(pg); all_phases.append(phases)
            if rc_o == 0:
                want_parts.append(want)
        asserted = np.array(asserted)
        assert b.n == 300 and 0 < asserted.sum() < 60
        b.upload(); b.run(); b.download()
        got = b.result()
        feats = {int(g): b.features(int(g)) for g in np.nonzero(~asserted)[0][:40]}
    assert (got.status[asserted] >= 100).all()
    batch = PackedGraphs.concat(want_parts)
    want = common.oracle_run(batch, threads=4)[0]
    sub = common.select_results(got, np.nonzero(~asserted)[0])
    assert not common.compare_results(want, sub, batch.n, conf_tol=1e-9)
    assert (want.status == 0).sum() > 200
    # the bulk form stages the same batch
    with A.DecompBatch(0) as b:
        b.add_packed_raw(PackedGraphs.concat(raws), 10000, all_phases); b.upload(); b.run(); b.download()
        again = b.result()
    assert not common.compare_results(got, again, 300)
    # features of raw graphs == features of the same graphs staged by the oracle's pre-steps
    with A.DecompBatch(0) as b:
        b.add(batch); b.upload(); b.run(); b.download()
        keep = np.nonzero(~asserted)[0]
        for k, g in enumerate(keep[:40]):
            assert [f.as_dict() for f in b.features(k)[0]] == [f.as_dict() for f in feats[int(g)][0]], g


def test_rccl_gather_behind_the_c_abi():
    """ald_comm_*: the exchange step for a multi-process host, in C behind the ABI (RCCL loaded on first use): unique id -> communicator ->
    gather of the finished-transcript streams to rank 0 -> ald_tset_add_stream.  One rank here (RCCL refuses two ranks on one device,
    and this box has one); run in a fresh process so that the library's RCCL and torch's bundled copy never share an address space."""
    import subprocess, sys, textwrap
    code = textwrap.dedent('''
        import ctypes as C, sys, numpy as np
        sys.path.insert(0, %r)
        import aletsch_amd as A
        lib = A.load_library()
        lib.ald_comm_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        lib.ald_comm_gather_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(C.c_int32))]
        lib.ald_comm_destroy.argtypes = [C.c_void_p]
        uid = (C.c_uint8 * 128)()
        assert lib.ald_comm_unique_id(uid) == 0, lib.ald_last_error()
        comm = C.c_void_p()
        assert lib.ald_comm_create(uid, 1, 0, 0, C.byref(comm)) == 0, lib.ald_last_error()
        pg = A.synth(seed=47, n_graphs=800, v_min=8, v_max=60, edges_per_vertex=3, layout_mode=1, weight_mode=2)
        sid = (np.arange(pg.n) %% 3).astype(np.int32)
        with A.DecompBatch(0) as b:
            b.add(pg); b.upload(); b.run(); b.download()
            w = b.transcript_stream(sid)
            direct = A.TranscriptSink(0.8); direct.add_batch(b, sid)
            for rep in range(3):                               # buffers are reused; the last round sends the stream built in HBM, from where it lies
                allw = C.POINTER(C.c_uint32)(); offs = C.POINTER(C.c_int64)(); goffs = C.POINTER(C.c_int32)()
                if rep < 2:
                    src, n = w.ctypes.data, w.size
                else:
                    src, n = b.device_transcript_stream(sid)
                    assert n == w.size
                assert lib.ald_comm_gather_streams(comm, C.c_void_p(src), C.c_int64(n), C.c_int32(0), C.byref(allw), C.byref(offs), C.byref(goffs)) == 0, lib.ald_last_error()
                assert offs[0] == 0 and offs[1] == w.size and goffs[0] == 0
                got = np.ctypeslib.as_array(allw, shape=(w.size,)).copy()
                assert np.array_equal(got, w), rep
        via = A.TranscriptSink(0.8); via.add_stream(got, graph_offset=int(goffs[0]))
        assert via.items() == direct.items() and len(via.items()) > 500
        assert lib.ald_comm_destroy(comm) == 0
        print("COMM_OK", w.size)
    ''') % common.ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "COMM_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_transcript_set_reduction_on_the_gpu():
    """ald_batch_reduce_transcripts: the batch's transcripts merged into an empty transcript_set ON THE DEVICE --
    item for item, field for field, bit for bit (coverage sums in the reference's nesting) what the host sink gives for the same batch
    (ald_tset_add_batch, itself pinned to the reference's transcript_set.cc).  The batch repeats graphs under different sample ids, so
    groups with many members, several samples per item and single-exon clusters all occur; then a second batch goes into the same
    persistent set through ald_tset_add_flat == transcript_set::add(set)."""
    from aletsch_amd.packed import PackedGraphs
    base = A.synth(seed=49, n_graphs=1500, v_min=6, v_max=60, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)
    rng = np.random.default_rng(5)
    pick = rng.integers(0, base.n, 4000)                                   # every graph ~2.7 times, shuffled: equal transcripts from different "samples"
    pg = base.select(pick)
    sid = rng.integers(-1, 6, pg.n).astype(np.int32)
    for skip in (False, True):
        with A.DecompBatch(0) as b:
            b.add(pg); b.upload(); b.run(); b.download()
            host = A.TranscriptSink(0.8); host.add_batch(b, sid, tid_base=3 << 44, skip_single_exon=skip)
            items, st = b.reduce_transcripts(sid, tid_base=3 << 44, skip_single_exon=skip)
        want = host.items()
        assert len(items) == len(want) and len(want) > 3000
        for a, w in zip(items, want):
            assert a == w, (skip, a, w)
        assert st["device_groups"] > 3000 and (skip or st["host_items"] > 0) and max(x["count"] for x in items) >= 3
        assert max(len(x["samples"]) for x in items) >= 3
    # two batches into one persistent set: each reduced on the device and merged set-into-set (ald_tset_add_flat), against the host path
    # doing the same with host-built sets (ald_tset_merge) -- both are transcript_set::add(transcript_set&), transcript_set.cc:156-175
    other = base.select(rng.integers(0, base.n, 1000)); sid2 = rng.integers(0, 6, other.n).astype(np.int32)
    import os
    for thr in (None, "7"):                                 # ald_tset_add_flat on one thread / on seven (one set of tables each)
        if thr:
            os.environ["ALD_SINK_THREADS"] = thr
        try:
            flat = A.TranscriptSink(0.8); ref = A.TranscriptSink(0.8)
            for part, s_, tb in ((pg, sid, 1 << 44), (other, sid2, 2 << 44)):
                with A.DecompBatch(0) as b:
                    b.add(part); b.upload(); b.run(); b.download()
                    if thr:
                        b.reduce_into(flat, s_, tid_base=tb)
                    else:
                        b.reduce_transcripts(s_, tid_base=tb, into=flat)
                    one = A.TranscriptSink(0.8); one.add_batch(b, s_, tid_base=tb)
                    ref.merge(one)
            assert flat.items() == ref.items() and len(ref.items()) > 3000
        finally:
            os.environ.pop("ALD_SINK_THREADS", None)


def test_transcript_stream_built_on_the_device():
    """ald_batch_device_transcript_stream leaves in HBM, word for word, the stream ald_batch_transcript_stream builds on the host
    (finished graphs only, exons joined, optional single-exon filter, sample ids) -- read back through a zero-copy tensor view"""
    import os
    import torch
    from aletsch_amd.distributed import _device_words
    pg = A.synth(seed=4242, n_graphs=3000, v_min=6, v_max=90, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)
    sid = (np.arange(pg.n) % 5).astype(np.int32)
    os.environ["ALD_DEBUG_UNDERCLASS"] = "1"            # abandoned capacity attempts in the raw pool: they must not show up
    try:
        with A.DecompBatch(0) as b:
            b.add(pg); b.upload(); b.run(); b.download()
            for skip in (False, True):
                for s in (sid, None):
                    want = b.transcript_stream(s, skip)
                    ptr, n = b.device_transcript_stream(s, skip)
                    assert n == want.size and n > 0
                    got = _device_words(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(np.uint32)
                    assert np.array_equal(got, want), (skip, s is None)
    finally:
        del os.environ["ALD_DEBUG_UNDERCLASS"]
    with A.DecompBatch(0) as b:                             # a batch without a single path
        b.add(A.synth(seed=5, n_graphs=3, v_min=2, v_max=2, edges_per_vertex=1)); b.upload(); b.run(); b.download()
        ptr, n = b.device_transcript_stream()
        assert n == b.transcript_stream().size


def test_result_index_written_by_the_kernel():
    """The kernel publishes, per graph that ended well, the pool offsets of its records in path order (one atomic per graph); the
    host never walks the record stream.  With every graph started one class too low the pool also holds the records of the abandoned
    attempts -- the index must not name them -- and every named record must be THE record of (graph, path): same vertices, same
    values as the exported result, exons = the oracle's transcripts."""
    import os
    from aletsch_amd.distributed import parse_records, REC_HDR_WORDS
    pg = A.synth(seed=4243, n_graphs=2500, v_min=6, v_max=90, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)
    os.environ["ALD_DEBUG_UNDERCLASS"] = "1"
    try:
        with A.DecompBatch(0) as b:
            b.add(pg); b.upload(); b.run(); b.download()
            r = b.result(); raw = b.raw_records(); idx, gf = b.result_index()
            cov, eo, lr = b.transcripts()
    finally:
        del os.environ["ALD_DEBUG_UNDERCLASS"]
    npaths = np.diff(r.path_offset)
    assert idx.size == int(npaths.sum()) and ((gf >= 0) == (npaths > 0)).all()
    allrec = parse_records(raw)
    assert len(allrec) >= idx.size                      # (records of abandoned attempts, if any were written before the overflow, are in the pool ...
    seen = set()
    for g in range(pg.n):
        for p in range(int(npaths[g])):
            o = int(idx[int(gf[g]) + p]); assert o not in seen; seen.add(o)
            assert int(raw[o]) == g and int(raw[o + 1]) == p
            i = int(r.path_offset[g]) + p
            nv = int(raw[o + 2]); nx = int(raw[o + 14])
            assert raw[o + REC_HDR_WORDS:o + REC_HDR_WORDS + nv].astype(np.int32).tolist() == r.path_vertices[int(r.pv_offset[i]):int(r.pv_offset[i + 1])].tolist()
            assert raw[o + 6:o + 8].view(np.float64)[0] == r.weight[i]
            assert raw[o + REC_HDR_WORDS + nv:o + REC_HDR_WORDS + nv + nx].astype(np.int32).reshape(-1, 2).tolist() == lr[int(eo[i]):int(eo[i + 1])].tolist()
    assert len(seen) == idx.size                        # ... and nothing names them)
    _, cov_o, eo_o, lr_o = common.oracle_transcripts(pg)
    assert np.array_equal(eo, eo_o) and np.array_equal(lr, lr_o) and np.array_equal(cov, cov_o)


def test_cfg4_rank0_shard_at_spec():
    """BASELINE configs[3] as one rank sees it: rank 0's shard of the 1 M-graph job, 125 000 x 64v/256e, seed 1004 + rank,
    against the oracle on all host cores.  (The other seven ranks run the same code on seeds 1005..1011; the merge of two such shards
    in rank order is tests/test_distributed_cpu.py::test_cfg4_shards_merge_in_rank_order.)"""
    pg = A.synth(seed=1004, n_graphs=125000, v_min=64, v_max=64, fixed_edges=256)
    got = A.decompose(pg, device=0)
    assert int((got.status != 0).sum()) == 0
    want = common.oracle_run(pg, threads=DR.THREADS)[0]
    assert not common.compare_results(want, got, pg.n, conf_tol=1e-9)


def _stream_of_groups(groups):
    """golden transcript groups (tests/golden/ref_tset.json) -> (transcript stream, coverage[], tid[])"""
    out = []; cov = []; tid = []
    for g, (sid, ts) in enumerate(groups):
        for k, (st, c, conf, abd, c1, t, ex) in enumerate(ts):
            hdr = np.zeros(12, np.uint32)
            hdr[0] = g; hdr[1] = k; hdr[2] = np.array([sid], np.int32).view(np.uint32)[0]; hdr[3] = ord(st); hdr[4] = c1; hdr[5] = len(ex)
            hdr[6:12] = np.array([0.0, conf, abd], np.float64).view(np.uint32)
            out.append(hdr); out.append(np.array([x for e in ex for x in e], np.int32).view(np.uint32)); cov.append(c); tid.append(t)
    return (np.concatenate(out) if out else np.zeros(0, np.uint32)), np.array(cov, np.float64), np.array(tid, np.int64)


def test_reference_tset_golden_through_the_device_reduction():
    """The six reference-generated cases of tests/golden/ref_tset.json (oracle/_ref/ref_tset = the reference's transcript_set.cc built
    from source) through the DEVICE stage of the reduction (ald_tset_reduce_stream: the same tx_* kernels a batch's records go through)
    -- every field of every merged item, bit for bit.  Before this the device reduction was only compared with the host sink."""
    import json
    import os
    import test_tset_cpu as T
    cases = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_tset.json")))
    n_dev = 0
    for c in cases:
        groups = T.as_groups(c)
        words, cov, tid = _stream_of_groups(groups)
        items, st = A.reduce_stream(words, coverage=cov, tid=tid)
        T.check(items, c["items"])
        n_dev += st["device_groups"]
        # and with the single-exon filter: the reference's own answer for the filtered input == filtering first
        items2, _ = A.reduce_stream(words, coverage=cov, tid=tid, skip_single_exon=True)
        s = A.TranscriptSink(0.8); s.add_groups(groups, skip_single_exon=True)
        assert items2 == s.items()
    assert n_dev > 100


def test_barrier_variant_of_the_hand_overs():
    """wsync() is a wavefront-scope fence (no instruction), so every lane-to-lane hand-over through LDS / the slabs relies on
    same-wave in-order memory.  libaletsch_decomp_wsync.so is the same source with __syncthreads() + an explicit s_waitcnt at every hand-over
    (make WSYNC=1: every memory counter waited for each time; until round 4 the compiler had lowered the __syncthreads() of a one-wave workgroup
    to nothing).  A fixed-seed fuzz slice through it against the oracle must be as clean as through the product
    build -- a divergence between the two forms would show here and not only in the ad-hoc fuzz tool.  Since round 4 the same build keeps
    the sweep records between sweeps in EVERY size class (-DALD_KEEP=1; the product: slab-resident classes only), so that the marks, the
    dense pass over the marked vertices and the prefetching scan -- device-only code -- run on every graph of the slice."""
    import subprocess, sys
    lib = os.path.join(common.ROOT, "aletsch_amd", "lib", "libaletsch_decomp_wsync.so")
    assert os.path.exists(lib), "build it with make -C aletsch_amd/csrc WSYNC=1 (python __graft_entry__.py does)"
    env = dict(os.environ, ALETSCH_DECOMP_LIB=lib, FUZZ_SECONDS="25", FUZZ_SEED="31337")
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "fuzz_parity.py")], capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("TOTAL graphs") and last.endswith("mismatches 0") and int(last.split()[2]) >= 1000, r.stdout[-1500:]


def test_register_form_of_the_small_fans_on_the_twins():
    """Round 4: the build that routes fans of 2..4 edges through star_reg instead of star_fixed (make STARREG=1) ended in a memory fault on
    the slab-resident twins: in that build the register allocator had placed four VGPR spills inside a two-instruction region of narrowed EXEC
    (profiles/r04/zb_slab_handover_drain.txt).  The source no longer has that region (ev_clear_marks) and the CPU tier searches the product's
    assembly for the pattern; this test keeps the build that exposed it in the GPU tier: 200 graphs of 385..512 vertices, every one forced
    onto the twins, through that build and through the product, against the oracle."""
    import subprocess, sys
    libs = [os.path.join(common.ROOT, "aletsch_amd", "lib", n) for n in ("libaletsch_decomp.so", "libaletsch_decomp_starreg.so")]
    assert os.path.exists(libs[1]), "build it with make -C aletsch_amd/csrc STARREG=1 (python __graft_entry__.py does)"
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "twins_parity.py"), *libs], capture_output=True, text=True, timeout=560)
    assert r.returncode == 0, r.stdout[-2500:] + r.stderr[-1500:]
    totals = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("TOTAL graphs")]
    assert len(totals) == 2 and all(ln.strip().endswith("mismatches 0") for ln in totals), r.stdout[-2500:]


def test_upload_stream_and_pinned_cache_knobs():
    """The three routings of ald_batch_upload's copies (ALD_UPLOAD_STREAM = 0 the batch's own stream, 1 / 2 a stream of the lowest / highest
    priority = default) and the pinned-block cache switched off (ALD_PINNED_CACHE_MB=0: every released block is a hipHostFree) give the same
    results: the twins' 200 graphs against the oracle in a child process per setting."""
    import subprocess, sys
    for env in ({"ALD_UPLOAD_STREAM": "0", "ALD_PINNED_CACHE_MB": "0"}, {"ALD_UPLOAD_STREAM": "1"}):
        r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "twins_parity.py")], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0 and "mismatches 0" in r.stdout, (env, r.stdout[-1500:] + r.stderr[-800:])


def test_row_form_of_the_kernels_on_gpu():
    """libaletsch_decomp_rows.so (make ROWS=1): the engine with adjacency rows in a segment pool -- whole-row reads by the wave, ballots
    for the position of an edge, merged edges placed by a merge of two sorted runs -- instead of linked lists.  The A/B build of round 4
    (slower than the list form: profiles/r04/); kept bit-exact: a fixed-seed fuzz slice against the oracle plus the bench shape."""
    import subprocess, sys
    lib = os.path.join(common.ROOT, "aletsch_amd", "lib", "libaletsch_decomp_rows.so")
    assert os.path.exists(lib), "build it with make -C aletsch_amd/csrc ROWS=1 (python __graft_entry__.py does)"
    env = dict(os.environ, ALETSCH_DECOMP_LIB=lib, FUZZ_SECONDS="25", FUZZ_SEED="4242")
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "fuzz_parity.py")], capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("TOTAL graphs") and last.endswith("mismatches 0") and int(last.split()[2]) >= 1000, r.stdout[-1500:]


def test_bench_line_and_its_exchange_path():
    """bench.py --full in a fresh process, as the driver starts it: ONE JSON line carrying the contract's keys, `roofline` and `cpu_baseline`; and
    once more with the multi-rank exchange forced on for the single rank this box has (ALD_BENCH_FORCE_DIST: process group over RCCL,
    transcript stream built on the device, gathered to rank 0, merged there) -- the path `--gpus N` takes on a multi-GPU node"""
    import json, os, subprocess, sys
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    for force in (False, True):
        e = dict(env, ALD_BENCH_FORCE_DIST="1") if force else env
        r = subprocess.run([sys.executable, os.path.join(common.ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--graphs", "20000", "--no-secondary",
                            "--cpu-sample", "0" if force else "2000", "--full"], capture_output=True, text=True, timeout=280, env=e)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        j = json.loads(lines[0])
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
            assert k in j, k
        assert j["metric"] == "bundles/sec" and j["value"] > 0 and j["n_gpus"] == 1 and j["steps"] == 3 and j["dtype"] == "f64" and j["vs_baseline"] is None
        assert j["roofline"]["bound"] == "hbm" and 0 < j["roofline"]["frac"] < 1 and j["config"]["failed_graphs"] == 0
        if not force:
            assert j["cpu_baseline"]["kind"] == "port" and j["cpu_baseline"]["value"] > 0


def test_bench_plain_run_and_its_outputs(tmp_path):
    """A plain bench.py run (no --full) times the headline loop only: the contract's keys, none of the figures that take runs of their
    own.  --dump-outputs writes what the last timed step computed, float64 and within 64 MB, the same in two runs, and the sampled
    graphs' path tables equal the oracle's decomposition of the same graphs."""
    import json, subprocess, sys
    from aletsch_amd.packed import DecompResult
    dumps = []
    for i in range(2):
        d = tmp_path / str(i)
        r = subprocess.run([sys.executable, os.path.join(common.ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--graphs", "20000",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        j = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
            assert k in j, k
        assert j["metric"] == "bundles/sec" and j["value"] > 0 and j["steps"] == 2 and j["value_is"] == "h2d_inclusive" and j["config"]["failed_graphs"] == 0
        assert not {"value_resident", "download_ms", "roofline", "secondary", "cpu_baseline", "cpu_baseline_1t"} & set(j), sorted(j)
        out = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert all(a.dtype == np.float64 for a in out.values()) and sum(a.nbytes for a in out.values()) <= 64 << 20
        dumps.append(out)
    a, b = dumps
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert len(a["status"]) == 20000 and (a["status"] == 0).all() and a["paths_per_graph"].sum() > 0
    g = a["sample_graph"].astype(np.int64)
    po = np.concatenate([[0], np.cumsum(a["sample_paths_per_graph"])]).astype(np.int32)
    got = DecompResult(status=a["status"][g].astype(np.int32), path_offset=po, weight=a["path_weight"], abd=a["path_abd"], conf=a["path_conf"],
                       reads=a["path_reads"], length=a["path_length"].astype(np.int32), count=a["path_count"].astype(np.int32),
                       strand=a["path_strand"].astype(np.int8), pv_offset=np.concatenate([[0], np.cumsum(a["path_n_vertices"])]).astype(np.int64),
                       path_vertices=a["path_vertices"].astype(np.int32))
    pg = A.synth(seed=1002, n_graphs=20000, v_min=64, v_max=64, fixed_edges=256)         # bench.py's workload at N = 1
    want = common.oracle_run(pg.select(g), threads=8)[0]
    bad = common.compare_results(want, got, len(g), conf_tol=1e-9)
    assert not bad, bad[:5]
