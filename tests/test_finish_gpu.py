"""GPU tier: ald_batch_finish -- a run ended on the device (status words, capacity retries, pool growth, the per-graph counters; no record
leaves HBM) -- and the three consumers that take a finished batch: the resident transcript set (ald_tset_dev_add_batch), the device-built
transcript stream and the batch-wide feature pass.  The yardstick is always the DOWNLOADED twin: a second DecompBatch over the same graphs
that ends with download(), and the host sink fed from it.  Every comparison is bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import aletsch_amd as A
import common
import shapes
from test_batch_features_gpu import assert_tables_equal, oracle_workload
from test_dev_tset_gpu import _arrays, _base
from test_features_raw_gpu import add_all_raw, random_extras, raw_draw
from test_gpu_adapter import graph_text

pytestmark = pytest.mark.gpu

ROOT = common.ROOT
ERR_STATE = -4


def finished(b, pg=None):
    if pg is not None:
        b.clear(); b.add(pg)
    b.upload(); b.run(); b.finish()
    return b


def downloaded(b, pg=None):
    if pg is not None:
        b.clear(); b.add(pg)
    b.upload(); b.run(); b.download()
    return b


def assert_items_equal(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for x, y in zip(got, want):
        assert x == y, (tag, x, y)


def device_words(b, sid=None, skip=False):
    import torch
    from aletsch_amd.distributed import _device_words
    ptr, n = b.device_transcript_stream(sid, skip)
    if n == 0:
        return np.zeros(0, np.uint32)
    return _device_words(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(np.uint32).copy()


def assert_same_table(got, want):
    """two features_all tables field by field, by bits (the padding of a row is not part of it; rows of a graph on which the reference would
    have asserted hold partial values, as in tests/test_batch_features_gpu.py)"""
    return assert_tables_equal(got, (want["rows"], want["complete"], want["graph_rc"], want["row_begin"]))


def code_of(call):
    with pytest.raises(A.DecompError) as e:
        call()
    return e.value.code


def test_set_equality_after_every_add():
    """the four re-selected batches of test_dev_tset_gpu.py (later batches land on earlier items, sids -1..7), both skip settings: the set
    fed from the finished batch == the set fed from the downloaded twin == the host sink, item for item, after EVERY add"""
    base = _base()
    rng = np.random.default_rng(11)
    parts = [base.select(rng.integers(0, base.n, k)) for k in (3000, 1000, 2500, 1500)]
    sids = [rng.integers(-1, 8, p.n).astype(np.int32) for p in parts]
    for skip in (False, True):
        host = A.TranscriptSink(0.8)
        with A.DeviceTranscriptSet(0, 0.8) as df, A.DeviceTranscriptSet(0, 0.8) as dd, A.DecompBatch(0) as bf, A.DecompBatch(0) as bd:
            for r, (pg, sid) in enumerate(zip(parts, sids)):
                finished(bf, pg); downloaded(bd, pg)
                assert bf.last_finish_ms()["bytes_to_host"] == 20 * pg.n + 16
                host.add_batch(bd, sid, tid_base=r << 44, skip_single_exon=skip)
                dd.add_batch(bd, sid, tid_base=r << 44, skip_single_exon=skip)
                df.add_batch(bf, sid, tid_base=r << 44, skip_single_exon=skip)
                lib = bf._lib                               # every export array of the three sets, FP64 by bits: item for item
                ng, got = _arrays(lib, lambda *a: lib.ald_tset_dev_size(df._h, *a), lambda *a: lib.ald_tset_dev_export(df._h, *a))
                nt, twin = _arrays(lib, lambda *a: lib.ald_tset_dev_size(dd._h, *a), lambda *a: lib.ald_tset_dev_export(dd._h, *a))
                nh, want = _arrays(lib, lambda *a: lib.ald_tset_size(host._h, *a), lambda *a: lib.ald_tset_export(host._h, *a))
                assert ng == nt == nh and nh > 3000, (skip, r, ng, nt, nh)
                for k, (x, y, z) in enumerate(zip(got, twin, want)):
                    assert np.array_equal(x, y) and np.array_equal(x, z), (skip, r, k)
            st = df.stats()
            assert st["device_items"] > 3000 and st["device_ms"] > 0
            assert (st["host_items"] == 0) if skip else (st["host_items"] > 0), st      # skip=False: the single-exon compaction ran
            assert st["host_items"] == dd.stats()["host_items"]


def test_only_single_exon_transcripts_and_nothing_at_all():
    pg = A.synth(seed=5, n_graphs=3, v_min=2, v_max=2, edges_per_vertex=1)
    with A.DecompBatch(0) as bf, A.DecompBatch(0) as bd:
        finished(bf, pg); downloaded(bd, pg)
        host = A.TranscriptSink(0.8); host.add_batch(bd)
        with A.DeviceTranscriptSet(0) as ds:
            ds.add_batch(bf)
            assert ds.items() == host.items() and len(host.items()) > 0 and ds.stats()["device_items"] == 0
        with A.DeviceTranscriptSet(0) as ds:
            ds.add_batch(bf, skip_single_exon=True)
            assert ds.size() == (0, 0, 0) and ds.items() == []
    with A.DecompBatch(0) as b:                             # no graph at all
        b.upload(); b.run(); b.finish()
        assert [len(a) for a in b.status_arrays()] == [0, 0, 0]
        t = b.features_all()
        assert len(t["rows"]) == 0 and t["row_begin"].tolist() == [0]
        assert device_words(b).size == 0
        with A.DeviceTranscriptSet(0) as ds:
            ds.add_batch(b)
            assert ds.size() == (0, 0, 0)


def _twin_check(pg, sid, reps=1):
    """status / path / iteration counts and the resident set of a finished batch against its downloaded twin -> the twin's status"""
    with A.DecompBatch(0) as bf, A.DecompBatch(0) as bd, A.DeviceTranscriptSet(0) as df, A.DeviceTranscriptSet(0) as dd:
        bf.add(pg); bf.upload(); bd.add(pg); bd.upload()
        for rep in range(reps):                             # (the second run of the resident batch uses what the first one grew)
            bf.run(); bf.finish(); bd.run(); bd.download()
            st, npth, nit = bf.status_arrays()
            res = bd.result()
            assert np.array_equal(st, res.status) and np.array_equal(npth, np.diff(res.path_offset)) and np.array_equal(nit, bd.iterations())
            for a, b2 in zip(bf.status_arrays(), bd.status_arrays()):
                assert np.array_equal(a, b2)
            df.add_batch(bf, sid, tid_base=rep << 44); dd.add_batch(bd, sid, tid_base=rep << 44)
            assert_items_equal(df.items(), dd.items(), rep)
            for skip in (False, True):
                assert np.array_equal(device_words(bf, sid, skip), device_words(bd, sid, skip))
        assert df.size()[0] > 0
        return st


def test_pool_growth_inside_finish(monkeypatch):
    """ALD_DEBUG_POOL_WORDS: ALD_ST_POOL_FULL -> finish grows the pool and the index and runs again; twice on the resident batch"""
    pg = A.synth(seed=33, n_graphs=600, v_min=20, v_max=90, edges_per_vertex=4)
    monkeypatch.setenv("ALD_DEBUG_POOL_WORDS", "5000")
    st = _twin_check(pg, (np.arange(pg.n) % 7 - 1).astype(np.int32), reps=2)
    assert (st == 0).all()


def test_capacity_retries_inside_finish(monkeypatch):
    """ALD_DEBUG_UNDERCLASS: the wide hubs outgrow the class they start in and finish re-queues them one class up.  The records of the
    abandoned attempts stay in the pool: nothing may read them"""
    pg = shapes.hub_batch()[0]
    monkeypatch.setenv("ALD_DEBUG_UNDERCLASS", "1")
    _twin_check(pg, (np.arange(pg.n) % 5).astype(np.int32))


def test_graphs_that_end_on_an_assert():
    pg = shapes.zero_count_batch()[0]
    with A.DecompBatch(0) as bf, A.DecompBatch(0) as bd, A.DeviceTranscriptSet(0) as ds:
        finished(bf, pg); downloaded(bd, pg)
        st, npth, _ = bf.status_arrays()
        assert (st >= 100).all() and np.array_equal(st, bd.result().status) and (npth == 0).all()
        ds.add_batch(bf)
        assert ds.size() == (0, 0, 0)
        assert device_words(bf).size == 0
        t = bf.features_all()
        assert len(t["rows"]) == 0 and t["row_begin"].tolist() == [0] * (pg.n + 1)


def test_stream_and_features():
    pg = A.synth(seed=45, n_graphs=400, v_min=8, v_max=60, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)
    sid = (np.arange(pg.n) % 5).astype(np.int32)
    with A.DecompBatch(0) as bf, A.DecompBatch(0) as bd:
        finished(bf, pg); downloaded(bd, pg)
        for skip in (False, True):
            for s in (sid, None):
                got, want = device_words(bf, s, skip), device_words(bd, s, skip)
                assert got.size > 0 and np.array_equal(got, want), (skip, s is None)
                assert np.array_equal(want, bd.transcript_stream(s, skip))
        # the feature pass on a staged batch
        pg2, extras = oracle_workload()
        finished(bf, pg2); downloaded(bd, pg2)
        got = bf.features_all(extras, g_nv=pg2.g_nv); want = bd.features_all(extras, g_nv=pg2.g_nv)
        assert len(want["rows"]) > 500 and got["stats"]["device_graphs"] == pg2.n
        assert_same_table(got, want)
        assert_same_table(bf.features_table(), want)
        # raw graphs: the host routine needs the downloaded records, the device pass does not
        items, _ = raw_draw(1076, 40)
        bf.clear(); bd.clear()
        g_nv = add_all_raw(bf, items); add_all_raw(bd, items)
        finished(bf); downloaded(bd)
        ex = random_extras(g_nv, np.random.default_rng(5))
        with pytest.raises(A.DecompError) as e:
            bf.features_all(ex, g_nv=g_nv)
        assert e.value.code == ERR_STATE and "ALD_FEAT_RAW_ON_DEVICE" in str(e.value)
        got = bf.features_all(ex, g_nv=g_nv, raw_on_device=True); want = bd.features_all(ex, g_nv=g_nv, raw_on_device=True)
        assert len(want["rows"]) > 40 and got["stats"]["host_graphs"] == 0
        assert_same_table(got, want)


def test_state_machine():
    base = _base()
    rng = np.random.default_rng(13)
    pg = base.select(rng.integers(0, base.n, 400)); sid = rng.integers(-1, 8, pg.n).astype(np.int32)
    with A.DecompBatch(0) as b, A.DecompBatch(0) as ran, A.DecompBatch(0) as twin:
        b.add(pg)
        assert code_of(b.finish) == ERR_STATE               # before upload
        b.upload()
        assert code_of(b.finish) == ERR_STATE               # before run
        assert code_of(b.status_arrays) == ERR_STATE
        b.run(); b.finish()
        assert b.last_finish_ms()["bytes_to_host"] == 20 * pg.n + 16
        first = [a.copy() for a in b.status_arrays()]
        b.finish()                                          # idempotent
        assert all(np.array_equal(x, y) for x, y in zip(first, b.status_arrays()))
        # what reads the host path table answers as for a batch that only ran
        ran.add(pg); ran.upload(); ran.run(); ran.sync()
        sink = A.TranscriptSink(0.8)
        for name, call in (("result", lambda x: x.result()), ("transcript_stream", lambda x: x.transcript_stream(sid)), ("raw_records", lambda x: x.raw_records()),
                           ("result_index", lambda x: x.result_index()), ("iterations", lambda x: x.iterations()), ("features", lambda x: x.features(0)),
                           ("reduce", lambda x: x.reduce_transcripts(sid)), ("sink", lambda x: sink.add_batch(x, sid))):
            assert code_of(lambda: call(b)) == code_of(lambda: call(ran)), name
        assert code_of(b.result) == ERR_STATE and sink.items() == []
        # finish(); download() == download() alone, and the download launches nothing
        k0 = b.kernel_ms()
        b.download()
        assert b.kernel_ms() == k0 > 0
        downloaded(twin, pg)
        assert not common.compare_results(twin.result(), b.result(), pg.n)
        assert all(np.array_equal(x, y) for x, y in zip(first, b.status_arrays()))
        assert np.array_equal(b.transcript_stream(sid), twin.transcript_stream(sid))
        b.finish()                                          # a downloaded batch has ended: nothing to do
        assert not common.compare_results(twin.result(), b.result(), pg.n)
        # upload / run reset the state as they reset `downloaded`
        b.run()
        assert code_of(b.status_arrays) == ERR_STATE
        b.finish(); b.upload()
        assert code_of(b.status_arrays) == ERR_STATE
    # a batch cleared and reused right after add_batch returns leaves the set correct
    with A.DeviceTranscriptSet(0) as ds, A.DecompBatch(0) as b, A.DecompBatch(0) as bd:
        host = A.TranscriptSink(0.8)
        for r in range(3):
            pg = base.select(rng.integers(0, base.n, 1200)); sid = rng.integers(-1, 8, pg.n).astype(np.int32)
            downloaded(bd, pg); host.add_batch(bd, sid, tid_base=r << 44)
            b.add(pg); b.upload(); b.run(); b.finish()
            ds.add_batch(b, sid, tid_base=r << 44)
            b.clear()
            b.add(A.synth(seed=900 + r, n_graphs=200, v_min=6, v_max=40, edges_per_vertex=3)); b.upload(); b.run(); b.finish(); b.clear()
        assert ds.items() == host.items()


def test_cpp_adapter_flush_on_device():
    """aletsch::gpu_scallop_batch::flush_on_device (tests/host_adapter/finish_test.cc): enqueue -> flush_on_device() ->
    ald_tset_dev_add_batch(handle()) gives the items of the flush() path; status(i) answers after either flush"""
    exe = os.path.join(ROOT, "tests", "_build", "finish_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    lib = os.path.join(ROOT, "aletsch_amd", "lib")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_adapter", "finish_test.cc"), "-o", exe, "-L" + lib, "-laletsch_decomp", "-Wl,-rpath," + lib], check=True)
    pg = A.synth(seed=63, n_graphs=40, v_min=3, v_max=40, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2)
    text = "%d\n" % pg.n + "".join(graph_text(pg.select(np.array([g]))) for g in range(pg.n))
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr)
    words = r.stdout.split()
    assert words[0] == "items" and int(words[1]) > 20 and words[-1] == "equal", r.stdout


def test_one_run_at_size():
    """one 100 000 x 64v/256e batch (the bench shape), skip_single_exon: the export arrays of the set fed from the finished batch equal,
    by bits, those of a second set fed from the same batch run again and downloaded"""
    n = 100000
    pg = A.synth(seed=1002, n_graphs=n, v_min=64, v_max=64, fixed_edges=256)
    sid = (np.arange(n) % 8).astype(np.int32)
    with A.DeviceTranscriptSet(0) as df, A.DeviceTranscriptSet(0) as dd, A.DecompBatch(0) as b:
        lib = b._lib
        b.add(pg); b.upload()
        b.run(); b.finish()
        fin = b.last_finish_ms()
        df.add_batch(b, sid, tid_base=1 << 44, skip_single_exon=True)
        b.run(); b.download()
        dd.add_batch(b, sid, tid_base=1 << 44, skip_single_exon=True)
        assert fin["bytes_to_host"] == 20 * n + 16 and b.download_ms()["bytes_to_host"] > 100 * fin["bytes_to_host"]
        nf, got = _arrays(lib, lambda *a: lib.ald_tset_dev_size(df._h, *a), lambda *a: lib.ald_tset_dev_export(df._h, *a))
        nd, want = _arrays(lib, lambda *a: lib.ald_tset_dev_size(dd._h, *a), lambda *a: lib.ald_tset_dev_export(dd._h, *a))
        assert nf == nd and nd > 100000
        for k, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), k
        assert df.stats()["host_items"] == 0
