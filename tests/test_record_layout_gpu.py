"""GPU tier of the record layout (aletsch_amd/csrc/record_layout.h): pairwise-distinct header words through every translation between a
path record and a transcript-stream record -- the kernels ts_emit, tp_emit, sr_emit and the host loops that call the same per-word
functions (ald_batch_transcript_stream, tx_stream_records), plus the readers of either format (ald_tset_add_stream, the front end).

The streams are built here with numpy by literal index, as the header's prose has the format: this file is an independent statement of
the ABI and never names a word through the library's constants.  Every comparison is exact."""
import functools
import math

import numpy as np
import pytest

import aletsch_amd as A
import common
from test_owner_split_cpu import split_model, walk

pytestmark = pytest.mark.gpu

EXONS = (1, 2, 8, 9, 17)          # 2, 4, 16, 18, 34 exon words: below, at and on both sides of the 16-lane copy stride
GRAPHS = ((3, 41), (4, -1), (9, 7))    # (graph id, sid): each graph a sample of its own, one of them the "no sample" -1
TID_BASE = 5 << 44


def one(graph, path, sid, strand, count1, weight, conf, abd, exons):
    h = np.zeros(12, np.uint32)
    h[0] = graph; h[1] = path; h[2] = np.uint32(sid & 0xFFFFFFFF); h[3] = ord(strand); h[4] = count1; h[5] = len(exons)
    h[6:8] = np.array([weight]).view(np.uint32); h[8:10] = np.array([conf]).view(np.uint32); h[10:12] = np.array([abd]).view(np.uint32)
    return np.concatenate([h, np.array(exons, np.int32).reshape(-1).view(np.uint32)])


@functools.lru_cache(maxsize=None)
def the_stream():
    """-> (words, [dict per transcript]): 3 graphs x 5 transcripts, every weight / conf / abd / count1 of the stream distinct, conf != abd.
    The 8-exon transcript of every graph has the SAME intron chain and strand (it merges across the three samples); all others are apart."""
    recs = []; parts = []
    for gi, (g, sid) in enumerate(GRAPHS):
        for pi, n in enumerate(EXONS):
            k = 5 * gi + pi
            base = 1000 if n == 8 else 100000 * (k + 1)
            ex = [(base + 300 * e, base + 300 * e + 100) for e in range(n)]
            if n == 8:                                    # same chain, own outer ends
                ex[0] = (ex[0][0] - 10 * gi, ex[0][1]); ex[-1] = (ex[-1][0], ex[-1][1] + 7 * gi)
            t = dict(graph=g, path=pi, sid=sid, strand="+" if n == 8 else "+-."[k % 3], count1=3 + k, weight=1.25 + 0.5 * k, conf=0.03125 * (k + 1), abd=100.5 + 3 * k, exons=ex)
            recs.append(t); parts.append(one(**t))
    vals = [x for t in recs for x in (t["weight"], t["conf"], t["abd"])]
    assert len(set(vals)) == len(vals) and len(set(t["count1"] for t in recs)) == len(recs)
    return np.concatenate(parts), recs


def without_single_exon(words):
    return np.concatenate([words[o:o + n] for o, n in walk(words) if int(words[o + 5]) > 1])


@pytest.mark.parametrize("skip", (False, True), ids=("all", "skip single-exon"))
def test_set_items_through_every_stream_reader(skip):
    """host pointer -> tx_stream_records; device pointer -> stream index + sr_emit; the host sink -> ald_tset_add_stream"""
    import torch
    words, recs = the_stream()
    with A.DeviceTranscriptSet(0, 0.8) as a, A.DeviceTranscriptSet(0, 0.8) as b:
        a.add_stream(words, graph_offset=2, tid_base=TID_BASE, skip_single_exon=skip)
        d = torch.from_numpy(words.view(np.int32).copy()).cuda(); torch.cuda.synchronize()
        b.add_stream_ptr(d.data_ptr(), words.size, graph_offset=2, tid_base=TID_BASE, skip_single_exon=skip)
        ia, ib = a.items(), b.items()
    host = A.TranscriptSink(0.8)
    host.add_stream(without_single_exon(words) if skip else words, graph_offset=2, tid_base=TID_BASE)   # (the host entry point has no filter of its own)
    ih = host.items(); host.close()
    assert ia == ih and ib == ih
    # and against the numbers the stream was built from: 13 items (the three 8-exon transcripts are one), less the 3 single-exon ones
    assert len(ih) == (10 if skip else 13)
    by_tid = {TID_BASE + (((t["graph"] + 2) << 20) | t["path"]): t for t in recs}
    merged = [x for x in ih if x["count"] > 1]
    assert len(merged) == 1 and merged[0]["count"] == 3 and len(merged[0]["exons"]) == 8
    for x in ih:
        if x["count"] == 1:
            t = by_tid[x["tid"]]
            assert x["strand"] == t["strand"] and x["conf"] == t["conf"] and x["abd"] == t["abd"] and x["count1"] == t["count1"] and x["exons"] == t["exons"]
            assert math.isclose(x["coverage"], math.log(1.0 + t["weight"]), rel_tol=1e-14) and x["cov2"] == x["coverage"]
            assert [s["sid"] for s in x["samples"]] == [t["sid"]] and x["samples"][0]["conf"] == t["conf"] and x["samples"][0]["abd"] == t["abd"]
    m = merged[0]; src = [t for t in recs if len(t["exons"]) == 8]
    assert m["conf"] == max(t["conf"] for t in src) and m["abd"] == max(t["abd"] for t in src) and m["count1"] == max(t["count1"] for t in src)
    assert sorted((s["sid"], s["conf"], s["abd"], s["count1"]) for s in m["samples"]) == sorted((t["sid"], t["conf"], t["abd"], t["count1"]) for t in src)


def test_split_of_the_stream():
    words, _ = the_stream()
    out, offs = A.split_stream(words, 1)
    assert list(offs) == [0, words.size] and np.array_equal(out, words)
    out, offs = A.split_stream(words, 3)
    want, woffs, _ = split_model(words, 3)
    assert np.array_equal(offs, woffs) and np.array_equal(out, want)
    assert all(woffs[r + 1] > woffs[r] for r in range(3))         # every owner got some of it


def device_words(ptr, n):
    import torch
    from aletsch_amd.distributed import _device_words
    if n == 0:
        return np.zeros(0, np.uint32)
    return _device_words(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(np.uint32).copy()


def test_streams_of_one_real_batch_agree_word_for_word():
    """host loop (ts_header_word per word), ts_emit, tp_emit -- and the test side's own restatement of the format"""
    pg = A.synth(seed=1212, n_graphs=8, v_min=32, v_max=32, fixed_edges=96)
    given = (np.arange(pg.n) * 3 - 1).astype(np.int32)            # -1, 2, 5, ...
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        r = b.result()
        assert int(np.diff(r.path_offset).sum()) > 50
        seen = set()
        for sid in (None, given):
            for skip in (False, True):
                want = common.transcript_stream_from_result(pg, r, sid, skip_single_exon=skip)
                host = b.transcript_stream(sid, skip)
                assert np.array_equal(host, want)
                p, n = b.device_transcript_stream(sid, skip)
                assert n == want.size and np.array_equal(device_words(p, n), want)
                p, offs = b.device_transcript_streams_by_owner(1, sid, skip)
                assert list(offs) == [0, want.size] and np.array_equal(device_words(p, want.size), want)
                seen.add(want.tobytes())
        assert len(seen) >= 2                                      # the sid reached the stream
