"""Transcripts that share hash buckets, on the GPU: the cases of tests/collide_cases.py through the reduction into an empty set
(tset_reduce.hip), the resident set fed host words and device words in every chunking (tset_resident.hip), the merge of two resident sets
and the split by bucket owner (tset_partition.hip).  Every comparison is against the items the reference's own transcript_set.cc printed
(tests/golden/ref_tset_collide.json.gz), bit for bit with check(); none is against the host sink."""
import functools

import numpy as np
import pytest

import aletsch_amd as A
import collide_cases as cc
from test_dev_stream_fold_gpu import Meta, to_device
from test_dev_tset_cpu import check
from test_dev_tset_gpu import stream_of
from test_owner_split_cpu import HDR, WORLDS, bucket_of, interleave, split_model, walk
from test_tset_collide_cpu import N_CASES, cut, golden

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def stream(i):
    groups, want = golden()[i]
    words, cov, tid = stream_of(groups, 0)
    return groups, want, words, cov, tid, Meta(words)


def chunks_of(i, chunk):
    """[(first word, end word, first transcript, end transcript)] of the stream cut every `chunk` groups"""
    groups, _, _, _, _, meta = stream(i)
    chunk = len(groups) if chunk == "all" else chunk
    out = []
    for a in range(0, len(groups), chunk):
        t0, t1 = (int(t) for t in np.searchsorted(meta.graph, [a, a + chunk]))
        out.append((int(meta.off[t0]), int(meta.off[t1]), t0, t1))
    return out


@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("i", range(N_CASES))
def test_reduction_into_an_empty_set(i, skip):
    _, want, words, cov, tid, _ = stream(i)
    items, st = A.reduce_stream(words, coverage=cov, tid=tid, skip_single_exon=skip)
    check(items, want["seq_multi" if skip else "seq"])
    assert (st["host_items"] == 0) == skip


@pytest.mark.parametrize("chunk", ("all", 7, 1))
@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("i", range(N_CASES))
def test_resident_set_fed_host_words(i, skip, chunk):
    _, want, words, cov, tid, _ = stream(i)
    with A.DeviceTranscriptSet(0, 0.8) as ds:
        for w0, w1, t0, t1 in chunks_of(i, chunk):
            ds.add_stream(words[w0:w1], coverage=cov[t0:t1], tid=tid[t0:t1], skip_single_exon=skip)
        check(ds.items(), want["seq_multi" if skip else "seq"])
        assert (ds.stats()["host_items"] == 0) == skip


@pytest.mark.parametrize("chunk", ("all", 7, 1))
@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("i", range(N_CASES))
def test_resident_set_fed_device_words(i, skip, chunk):
    _, want, words, cov, tid, meta = stream(i)
    dev = to_device(words)
    with A.DeviceTranscriptSet(0, 0.8) as ds:
        for w0, w1, t0, t1 in chunks_of(i, chunk):
            ds.add_stream_ptr(dev.data_ptr() + 4 * w0, w1 - w0, coverage=cov[t0:t1], tid=tid[t0:t1], skip_single_exon=skip)
            if w1 > w0:
                assert ds.stream_stats()["words_to_host"] == 0
                meta.check_stats(ds.stream_stats(), t0, t1, skip)
        check(ds.items(), want["seq_multi" if skip else "seq"])


@pytest.mark.parametrize("parts", (2, 3))
@pytest.mark.parametrize("i", range(N_CASES))
def test_merge_of_resident_sets(i, parts):
    """device sets built from the segments and folded left to right with ald_tset_dev_merge: the reference's transcript_set::add(transcript_set&)
    of its own sets; the source is left empty; the snapshot fed into an empty host sink gives the same items"""
    groups, want, _, _, _, _ = stream(i)
    sets = [A.DeviceTranscriptSet(0, 0.8) for _ in range(parts)]
    try:
        a = 0
        for ds, seg in zip(sets, cut(groups, parts)):
            w, c, t = stream_of(seg, a); a += len(seg)
            ds.add_stream(w, coverage=c, tid=t)
            assert ds.size()[0] > 100
        for ds in sets[1:]:
            sets[0].merge(ds)
            assert ds.size() == (0, 0, 0) and ds.items() == []
        check(sets[0].items(), want["merge%d" % parts])
        flat = A.TranscriptSink(0.8); sets[0].snapshot_into(flat)
        check(flat.items(), want["merge%d" % parts])
    finally:
        for ds in sets:
            ds.close()


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("i", range(N_CASES))
def test_owner_split(i, world):
    """the split against split_model word for word; every transcript of a bucket with one owner; every sub-stream folded into a resident set
    of its own; the owners' items ordered by hash, each owner's order inside a bucket kept, are the reference's items, ids included"""
    _, want, words, cov, tid, _ = stream(i)
    out, offs = A.split_stream(words, world)
    model, moffs, order = split_model(words, world)
    assert np.array_equal(offs, moffs) and np.array_equal(out, model)
    order = np.array(order, np.int64); starts = np.cumsum([0] + [n for _, n in walk(out)])
    parts = []; owner_of = {}
    for r in range(world):
        seg = out[offs[r]:offs[r + 1]]
        mine = order[(starts[:-1] >= offs[r]) & (starts[:-1] < offs[r + 1])]
        assert len(mine) == len(walk(seg)) > 0
        for o, n in walk(seg):
            assert owner_of.setdefault(bucket_of(seg[o + HDR:o + n].view(np.int32)), r) == r
        with A.DeviceTranscriptSet(0, 0.8) as ds:
            ds.add_stream(seg, coverage=cov[mine], tid=tid[mine])
            parts.append(ds.items())
        assert all(x["hash"] % world == r for x in parts[-1])
    check(interleave(parts), want["seq"])
