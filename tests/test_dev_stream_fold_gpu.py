"""A transcript stream in DEVICE memory folded into the resident set without a host walk (ald_tset_dev_add_stream on a device pointer:
stream index, sr_len / sr_emit, then the fold a finished batch takes): the reference's golden cases in every chunking, real weights from a
decomposed batch, groups whose transcripts the filter leaves out, refused streams, and ald_tset_split_stream device to device.  After every
device-pointer call the set reports that no stream word reached the host and how many bytes did.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import aletsch_amd as A
from stream_cases import DECOYS, MALFORMED, WELL_FORMED
from test_dev_tset_cpu import as_groups, check
from test_dev_tset_gpu import GOLDEN, stream_of
from test_owner_split_cpu import walk
from test_owner_split_gpu import assert_split, chain, one

pytestmark = pytest.mark.gpu
ERR_INVALID = -1


class Meta:
    """per-transcript facts of a stream by the host walk, as prefix sums: what a call on transcripts [t0, t1) may bring to the host"""

    def __init__(self, words):
        recs = walk(words)
        self.off = np.array([o for o, _ in recs] + [len(words)], np.int64)
        self.graph = words[self.off[:-1]].astype(np.int64) if recs else np.zeros(0, np.int64)
        k = 2 * words[self.off[:-1] + 5].astype(np.int64) if recs else np.zeros(0, np.int64)
        single = k <= 2
        self.n_single = np.concatenate([[0], np.cumsum(single)])
        self.single_words = np.concatenate([[0], np.cumsum(np.where(single, 18 + k, 0))])      # their compacted records: 16 + 2 vertices + k words
        head = np.ones(len(recs), bool); head[1:] = self.graph[1:] != self.graph[:-1]
        self.head = head

    def check_stats(self, st, t0, t1, skip):
        nt = t1 - t0
        singles = int(self.n_single[t1] - self.n_single[t0])
        kept = nt - singles if skip else nt
        h = self.head[t0:t1].copy()
        if nt:
            h[0] = True
        groups = int(h.sum())
        bound = 24 * kept + 16 * groups + (0 if skip else 4 * int(self.single_words[t1] - self.single_words[t0])) + 4096
        assert st["words_to_host"] == 0 and st["n_transcripts"] == nt and st["n_graphs"] == groups, (st, nt, groups)
        assert st["bytes_to_host"] <= bound, (st, kept, groups, bound)


def to_device(words):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return t


@functools.lru_cache(maxsize=None)
def golden_stream(i):
    groups = as_groups(GOLDEN[i][0])
    words, cov, tid = stream_of(groups, 0)
    return groups, words, cov, tid, Meta(words)


@pytest.mark.parametrize("chunk", ("all", 7, 1))
@pytest.mark.parametrize("skip", (False, True))
@pytest.mark.parametrize("i", range(len(GOLDEN)))
def test_golden_cases_through_a_device_pointer(i, skip, chunk):
    """test_golden_pin_every_chunking's chunkings (all groups, 7, 1), but every chunk folded where it lies in HBM, coverage / tid given, both
    skip settings: the reference's items (with the filter: the host sink's), and the items of the host-pointer add_stream of the same chunks"""
    groups, words, cov, tid, meta = golden_stream(i)
    dev = to_device(words)
    want_skip = None
    if skip:
        host = A.TranscriptSink(0.8); host.add_groups(groups, skip_single_exon=True)
        want_skip = host.items()
    chunk = max(len(groups), 1) if chunk == "all" else chunk
    with A.DeviceTranscriptSet(0, 0.8) as ds, A.DeviceTranscriptSet(0, 0.8) as hs:
        for a in range(0, max(len(groups), 1), chunk):
            t0, t1 = np.searchsorted(meta.graph, [a, a + chunk])
            w0, w1 = int(meta.off[t0]), int(meta.off[t1])
            ds.add_stream_ptr(dev.data_ptr() + 4 * w0, w1 - w0, coverage=cov[t0:t1], tid=tid[t0:t1], skip_single_exon=skip)
            if w1 > w0:
                meta.check_stats(ds.stream_stats(), int(t0), int(t1), skip)
            hs.add_stream(words[w0:w1], coverage=cov[t0:t1], tid=tid[t0:t1], skip_single_exon=skip)
            assert hs.stream_stats()["words_to_host"] == 0
        got = ds.items()
        if skip:
            assert got == want_skip and ds.stats()["host_items"] == 0
        else:
            check(got, GOLDEN[i][1])
        assert got == hs.items()


def test_real_weights_in_three_parts():
    """a decomposed batch's stream cut at graph boundaries, ids rebased to 0, no coverage[] / tid[]: log(1 + weight) on the host's libm
    under the sort, ids from graph_offset -- equal to the host sink fed the same parts"""
    pg = A.synth(seed=49, n_graphs=1500, v_min=6, v_max=60, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)
    sid = np.random.default_rng(17).integers(-1, 8, pg.n).astype(np.int32)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        for skip in (False, True):
            stream = b.transcript_stream(sid, skip)
            meta = Meta(stream)
            cuts = [0] + [int(np.searchsorted(meta.graph, g)) for g in (500, 1000)] + [len(meta.graph)]
            host = A.TranscriptSink(0.8)
            with A.DeviceTranscriptSet(0, 0.8) as ds:
                for t0, t1 in zip(cuts[:-1], cuts[1:]):
                    assert t1 > t0
                    first = int(meta.graph[t0])
                    part = stream[meta.off[t0]:meta.off[t1]].copy()
                    part[meta.off[t0:t1] - meta.off[t0]] -= np.uint32(first)
                    dev = to_device(part)
                    ds.add_stream_ptr(dev.data_ptr(), part.size, graph_offset=first, skip_single_exon=skip)
                    meta.check_stats(ds.stream_stats(), t0, t1, skip)
                    assert ds.stream_stats()["index_ms"] > 0
                    host.add_stream(part, graph_offset=first)
                got, want = ds.items(), host.items()
            assert len(got) == len(want) > 1000
            for x, y in zip(got, want):
                assert x == y, (skip, x, y)
            assert skip or any(len(x["exons"]) == 1 for x in want)
            assert len({x["coverage"] for x in want}) > 100                # real weights, not a constant


def test_groups_are_counted_before_the_filter():
    """three runs, the middle one single-exon only, the filter on: the middle run still takes a group number (labels and sample ids of the
    third run would shift otherwise), and the first transcript of a run gives the run's sample id even when it is itself left out"""
    words = np.concatenate([
        one(4, 0, [(100, 900)], sid=3), one(4, 1, chain(3, 1000), sid=5), one(4, 2, chain(4, 5000), sid=6),
        one(6, 0, [(20000, 20500)], sid=1), one(6, 1, [(40000, 40100)], sid=2), one(6, 2, [], sid=2),
        one(9, 0, chain(3, 1000), sid=7, weight=2.5), one(9, 1, [(70000, 70900)], sid=0), one(9, 2, chain(4, 5000), sid=0, weight=0.25), one(9, 3, chain(2, 300), sid=4)])
    meta = Meta(words); dev = to_device(words)
    for skip in (True, False):
        with A.DeviceTranscriptSet(0, 0.8) as ds, A.DeviceTranscriptSet(0, 0.8) as hs:
            for rnd in range(2):                                            # the second round lands on the items of the first
                ds.add_stream_ptr(dev.data_ptr(), words.size, graph_offset=11, tid_base=rnd << 40, skip_single_exon=skip)
                meta.check_stats(ds.stream_stats(), 0, 10, skip)
                hs.add_stream(words, graph_offset=11, tid_base=rnd << 40, skip_single_exon=skip)
            got = ds.items()
            assert got == hs.items() and (len(got) == 3 if skip else len(got) > 3)
            if skip:
                assert sorted(x["tid"] for x in got) == sorted(((g + 11) << 20) | p for g, p in ((4, 1), (4, 2), (9, 3)))
                assert {s["sid"] for x in got for s in x["samples"]} == {3, 7}      # the runs' first transcripts: left out (run 4) or not (run 9)


def test_refused_streams_leave_the_set_as_it_was():
    groups, words, cov, tid, meta = golden_stream(4)
    dev = to_device(words)
    with A.DeviceTranscriptSet(0, 0.8) as ds:
        ds.add_stream_ptr(dev.data_ptr(), words.size, coverage=cov, tid=tid)
        before = ds.items(); size = ds.size()
        assert len(before) >= 3 and size[0] == len(before)
        for name in sorted(MALFORMED):
            bad = to_device(MALFORMED[name][0])
            for skip in (False, True):
                with pytest.raises(A.DecompError) as e:
                    ds.add_stream_ptr(bad.data_ptr(), MALFORMED[name][0].size, skip_single_exon=skip)
                assert e.value.code == ERR_INVALID, name
                assert ds.stream_stats()["words_to_host"] == 0 and ds.size() == size, name
        assert ds.items() == before
        check(before, GOLDEN[4][1])


@pytest.mark.parametrize("name", ["200 exons among 2", "5000 exons among 2", "5000 exons first", "200 exons last", "chain of 4097"] + list(DECOYS))
def test_split_of_a_device_stream(name):
    for world in (3, 8):
        assert_split(WELL_FORMED[name], world, src_dev=True, dst_dev=True)
