"""The resident transcript set (ald_tset_dev_*, aletsch_amd/csrc/tset_resident.hip) on the GPU: batches and streams folded into a set
that stays in HBM, against the reference's own transcript_set.cc (tests/golden/ref_tset.json, ref_tset_resident.json.gz) and against
the host sink (ald_tset_add_batch / ald_tset_merge, itself pinned to the reference).  ref_tset_resident.json.gz stores the
reference's answers; its groups are drawn again from the seed (tests/golden/make_golden_dev_tset.py).  Every comparison is bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import aletsch_amd as A
from test_dev_tset_cpu import as_groups, check, mk

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = [(c["groups"], c["items"]) for c in json.load(open(os.path.join(HERE, "golden", "ref_tset.json")))] + mk.load()


def stream_of(groups, first):
    """groups (as_groups form) -> transcript stream words (graph id = first + position), coverage[], tid[] in stream order"""
    words = []; cov = []; tid = []
    for g, (sid, ts) in enumerate(groups):
        for p, (st, c, conf, abd, c1, t, ex) in enumerate(ts):
            hdr = np.zeros(12, np.uint32)
            hdr[0] = first + g; hdr[1] = p; hdr[2] = np.uint32(sid & 0xFFFFFFFF); hdr[3] = ord(st); hdr[4] = c1; hdr[5] = len(ex)
            hdr[6:8] = np.array([0.0]).view(np.uint32); hdr[8:10] = np.array([conf]).view(np.uint32); hdr[10:12] = np.array([abd]).view(np.uint32)
            words.append(hdr); words.append(np.array(ex, np.int32).reshape(-1).view(np.uint32))
            cov.append(c); tid.append(t)
    if not words:
        return np.zeros(0, np.uint32), np.zeros(0), np.zeros(0, np.int64)
    return np.concatenate(words), np.array(cov, np.float64), np.array(tid, np.int64)


def feed(ds, groups, chunk, skip):
    for a in range(0, max(len(groups), 1), chunk):
        w, c, t = stream_of(groups[a:a + chunk], a)
        ds.add_stream(w, coverage=c, tid=t, skip_single_exon=skip)


@pytest.mark.parametrize("i", range(len(GOLDEN)))
def test_golden_pin_every_chunking(i):
    """the reference's items after the last chunk, whatever the cut: one call, chunks of 7 groups, one call per group -- so groups keep
    landing on items that earlier calls made, and the resident start of the coverage sums is pinned to the reference's object code"""
    groups, items = GOLDEN[i]; groups = as_groups(groups)
    for chunk in (len(groups), 7, 1):
        with A.DeviceTranscriptSet(0, 0.8) as ds:
            feed(ds, groups, chunk, False)
            check(ds.items(), items)
    host = A.TranscriptSink(0.8); host.add_groups(groups, skip_single_exon=True)
    want = host.items()
    for chunk in (len(groups), 7):
        with A.DeviceTranscriptSet(0, 0.8) as ds:
            feed(ds, groups, chunk, True)
            assert ds.items() == want and ds.stats()["host_items"] == 0


def _base():
    return A.synth(seed=49, n_graphs=1500, v_min=6, v_max=60, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)


def test_batches_against_the_host_sink_after_every_add():
    """four batches re-selected from a common base (later batches hit earlier items; many samples per item); sids -1..7, both skip
    settings; the device set equals the host sink after EVERY add"""
    base = _base()
    rng = np.random.default_rng(11)
    parts = [base.select(rng.integers(0, base.n, k)) for k in (3000, 1000, 2500, 1500)]
    sids = [rng.integers(-1, 8, p.n).astype(np.int32) for p in parts]
    for skip in (False, True):
        host = A.TranscriptSink(0.8)
        with A.DeviceTranscriptSet(0, 0.8) as ds, A.DecompBatch(0) as b:
            for r, (pg, sid) in enumerate(zip(parts, sids)):
                b.clear(); b.add(pg); b.upload(); b.run(); b.download()
                host.add_batch(b, sid, tid_base=r << 44, skip_single_exon=skip)
                ds.add_batch(b, sid, tid_base=r << 44, skip_single_exon=skip)
                got, want = ds.items(), host.items()
                assert len(got) == len(want) and len(want) > 3000
                for x, y in zip(got, want):
                    assert x == y, (skip, r, x, y)
            st = ds.stats()
            assert st["device_items"] > 3000 and (skip or st["host_items"] > 0) and st["device_ms"] > 0
        assert max(x["count"] for x in want) >= 6 and max(len(x["samples"]) for x in want) >= 5


def _gtf(items):
    return "".join(A.format_transcript("chr1", "aletsch", "g%d" % k, "t%d" % x["tid"], x["strand"], x["coverage"], x["exons"], x["cov2"], x["count"])
                   for k, x in enumerate(items))


def test_merge_and_snapshot():
    """two device sets merged == ald_tset_merge of their host twins, src left empty; snapshot -> ald_tset_add_flat into an empty host set
    == the host sink, and the GTF records written from both are byte for byte the same"""
    base = _base()
    rng = np.random.default_rng(12)
    with A.DeviceTranscriptSet(0) as d1, A.DeviceTranscriptSet(0) as d2, A.DecompBatch(0) as b:
        h1 = A.TranscriptSink(0.8); h2 = A.TranscriptSink(0.8)
        for r in range(4):
            pg = base.select(rng.integers(0, base.n, 1500)); sid = rng.integers(-1, 8, pg.n).astype(np.int32)
            b.clear(); b.add(pg); b.upload(); b.run(); b.download()
            d, h = (d1, h1) if r % 2 == 0 else (d2, h2)
            d.add_batch(b, sid, tid_base=r << 44); h.add_batch(b, sid, tid_base=r << 44)
        d1.merge(d2); h1.merge(h2)
        want = h1.items()
        assert d1.items() == want and len(want) > 3000
        assert d2.size() == (0, 0, 0) and d2.items() == []
        flat = A.TranscriptSink(0.8); d1.snapshot_into(flat)
        got = flat.items()
        assert got == want
        assert _gtf(got) == _gtf(want)


@pytest.mark.parametrize("shape", ("device part only", "both parts", "host part only", "empty"))
def test_the_four_shapes_of_a_snapshot(shape):
    """snapshot() has a device part, a host part (fewer than two exons), both or neither.  Collide case 0 -- single-exon items and chains
    share buckets there -- with and without the single-exon filter, its single-exon transcripts alone, and an empty stream: the export of
    the resident set, its snapshot zipped into an empty host sink and the reduction into an empty set give the same items, which are the
    reference's stored ones (for the host part alone: a host sink's, which the CPU tier pins to the reference)"""
    from test_tset_collide_cpu import golden
    groups, want = golden()[0]
    singles = [g for g in ((sid, [t for t in ts if len(t[6]) == 1]) for sid, ts in groups) if g[1]]
    gs, skip = {"device part only": (groups, True), "both parts": (groups, False), "host part only": (singles, False), "empty": ([], False)}[shape]
    w, c, t = stream_of(gs, 0)
    with A.DeviceTranscriptSet(0, 0.8) as ds:
        ds.add_stream(w, coverage=c, tid=t, skip_single_exon=skip)
        exported = ds.items(); st = ds.stats(); size = ds.size()
        flat = A.TranscriptSink(0.8); ds.snapshot_into(flat)
    reduced, _ = A.reduce_stream(w, coverage=c, tid=t, skip_single_exon=skip)
    assert exported == flat.items() and exported == reduced
    assert (st["device_items"] > 0) == (shape in ("device part only", "both parts")) and (st["host_items"] > 0) == (shape in ("both parts", "host part only"))
    assert size[0] == len(exported) and size[1] == sum(len(x["exons"]) for x in exported) and size[2] == sum(len(x["samples"]) for x in exported)
    if shape == "empty":
        assert exported == [] and size == (0, 0, 0)
    elif shape == "host part only":
        host = A.TranscriptSink(0.8); host.add_groups(singles)
        assert exported == host.items() and len(exported) > 0
    else:
        check(exported, want["seq_multi" if skip else "seq"])


def test_edge_cases():
    import ctypes
    base = _base()
    rng = np.random.default_rng(13)
    with A.DeviceTranscriptSet(0) as ds:
        # no multi-exon path (graphs of two vertices: one single-exon transcript each, left out) and an empty stream change nothing;
        # without the filter the single-exon transcripts reach the host part
        with A.DecompBatch(0) as b:
            b.add(A.synth(seed=5, n_graphs=3, v_min=2, v_max=2, edges_per_vertex=1)); b.upload(); b.run(); b.download()
            ds.add_batch(b, skip_single_exon=True)
            ds.add_stream(np.zeros(0, np.uint32))
            assert ds.size() == (0, 0, 0) and ds.items() == []
            with A.DeviceTranscriptSet(0) as singles:
                host = A.TranscriptSink(0.8); host.add_batch(b); singles.add_batch(b)
                assert singles.items() == host.items() and singles.stats()["device_items"] == 0
        # ALD_ERR_STATE for a batch that ran but was not downloaded
        pg = base.select(rng.integers(0, base.n, 400)); sid = rng.integers(-1, 8, pg.n).astype(np.int32)
        with A.DecompBatch(0) as b:
            b.add(pg); b.upload(); b.run(); b.sync()
            with pytest.raises(A.DecompError) as e:
                ds.add_batch(b, sid)
            assert e.value.code == -4
            b.download()
            # growth past the first allocation: a small batch, then a large one; re-adding the same batch keeps the items, doubles the counts
            host = A.TranscriptSink(0.8)
            ds.add_batch(b, sid, skip_single_exon=True); host.add_batch(b, sid, skip_single_exon=True)
            small = ds.size()
            big = base.select(rng.integers(0, base.n, 6000)); bsid = rng.integers(-1, 8, big.n).astype(np.int32)
            b.clear(); b.add(big); b.upload(); b.run(); b.download()
            ds.add_batch(b, bsid, tid_base=1 << 44, skip_single_exon=True); host.add_batch(b, bsid, tid_base=1 << 44, skip_single_exon=True)
            assert ds.size()[0] > small[0] and ds.items() == host.items()
        with A.DeviceTranscriptSet(0) as once:
            with A.DecompBatch(0) as b:
                b.add(pg); b.upload(); b.run(); b.download()
                once.add_batch(b, sid, skip_single_exon=True)
                first = once.items()
                once.add_batch(b, sid, skip_single_exon=True)
            again = once.items()
            assert len(again) == len(first) > 0 and [x["count"] for x in again] == [2 * x["count"] for x in first]
        # a batch cleared and reused right after add_batch returns leaves the set correct
        with A.DeviceTranscriptSet(0) as ds2, A.DecompBatch(0) as b:
            host = A.TranscriptSink(0.8)
            for r in range(3):
                pg = base.select(rng.integers(0, base.n, 1200)); sid = rng.integers(-1, 8, pg.n).astype(np.int32)
                b.add(pg); b.upload(); b.run(); b.download()
                host.add_batch(b, sid, tid_base=r << 44)
                ds2.add_batch(b, sid, tid_base=r << 44)
                b.clear()
                b.add(A.synth(seed=900 + r, n_graphs=200, v_min=6, v_max=40, edges_per_vertex=3)); b.upload(); b.run(); b.download(); b.clear()
            assert ds2.items() == host.items()


def _arrays(lib, size_fn, export_fn):
    n = C.c_int64(); ne = C.c_int64(); ns = C.c_int64()
    assert size_fn(C.byref(n), C.byref(ne), C.byref(ns)) == 0
    n, ne, ns = n.value, ne.value, ns.value
    z = lambda k, dt: np.zeros(max(k, 1), dt)
    arrs = [z(n, np.uint64), z(n, np.int32), z(n, np.int8), z(n, np.float64), z(n, np.float64), z(n, np.float64), z(n, np.float64), z(n, np.int32), z(n, np.int32),
            z(n, np.int64), z(n + 1, np.int64), z(2 * ne, np.int32), z(n + 1, np.int64), z(ns, np.int32), z(ns, np.float64), z(ns, np.float64), z(ns, np.float64), z(ns, np.int32)]
    assert export_fn(*[C.c_void_p(x.ctypes.data) for x in arrs]) == 0
    return n, [a.view(np.uint64) if a.dtype == np.float64 else a for a in arrs]          # FP64 compared by bits


def test_full_size_batches_equal_the_host_sink():
    """three 100 000 x 64v/256e batches (the bench shape): the same graphs twice under other sample ids, then fresh graphs"""
    n = 100000
    pg1 = A.synth(seed=1002, n_graphs=n, v_min=64, v_max=64, fixed_edges=256)
    pg3 = A.synth(seed=1003, n_graphs=n, v_min=64, v_max=64, fixed_edges=256)
    host = A.TranscriptSink(0.8)
    with A.DeviceTranscriptSet(0) as ds, A.DecompBatch(0) as b:
        lib = b._lib
        for r, (pg, sid) in enumerate(((pg1, np.arange(n) % 8), (pg1, (np.arange(n) + 3) % 8), (pg3, np.arange(n) % 8))):
            sid = sid.astype(np.int32)
            b.clear(); b.add(pg); b.upload(); b.run(); b.download()
            host.add_batch(b, sid, tid_base=r << 44, skip_single_exon=True)
            ds.add_batch(b, sid, tid_base=r << 44, skip_single_exon=True)
        nd, got = _arrays(lib, lambda *a: lib.ald_tset_dev_size(ds._h, *a), lambda *a: lib.ald_tset_dev_export(ds._h, *a))
        nh, want = _arrays(lib, lambda *a: lib.ald_tset_size(host._h, *a), lambda *a: lib.ald_tset_export(host._h, *a))
        assert nd == nh and nd > 1000000
        for k, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), k
        assert ds.stats()["device_ms"] > 0
