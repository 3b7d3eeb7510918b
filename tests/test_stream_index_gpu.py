"""The stream index on the GPU (aletsch_amd/csrc/tset_index.hip): ald_tset_index_stream against the host walk word for word -- chain lengths
around every round of the pointer doubling, long records among short ones, payloads that read as record headers, every stream the other
tests use, the streams the walk refuses -- with the source and the offsets each in host and in device memory.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import aletsch_amd as A
from stream_cases import CHAIN_LENGTHS, DECOYS, MALFORMED, WELL_FORMED, runs
from test_dev_tset_cpu import as_groups
from test_dev_tset_gpu import stream_of
from test_owner_split_cpu import GOLDEN, walk
from test_owner_split_gpu import EDGE_STREAMS

pytestmark = pytest.mark.gpu
ERR_INVALID = -1
PLACES = [(s, d) for s in (False, True) for d in (False, True)]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(offsets, runs) of a named stream by the host walk, computed once"""
    w = stream(name)
    return np.array([o for o, _ in walk(w)] + [len(w)], np.int64), runs(w)


def stream(name):
    if name.startswith("golden "):
        return golden(int(name.split()[1]))
    return WELL_FORMED[name] if name in WELL_FORMED else EDGE_STREAMS[name]


@functools.lru_cache(maxsize=None)
def golden(i):
    return stream_of(as_groups(GOLDEN[i][0]), 0)[0]


def run_index(words, src_dev, dst_dev, capacity=None):
    """ald_tset_index_stream -> (offsets[capacity], nt, ng); raises DecompError (with .counts) as the binding does"""
    import torch
    words = np.ascontiguousarray(words, np.uint32); n = words.size
    cap = n // 12 + 2 if capacity is None else capacity
    keep = []
    if src_dev and n:
        t = torch.from_numpy(words.view(np.int32).copy()).cuda(); keep.append(t); src = t.data_ptr()
    else:
        src = words.ctypes.data
    offs = np.full(max(cap, 1), -7, np.int64)
    if dst_dev:
        d = torch.full((max(cap, 1),), -7, dtype=torch.int64, device="cuda"); dst = d.data_ptr()
    else:
        dst = offs
    torch.cuda.synchronize()
    nt, ng = A.index_stream_into(src, n, dst, cap)
    if dst_dev:
        offs = d.cpu().numpy()
    return offs, nt, ng


def assert_index(name):
    want, want_runs = expected(name)
    for src_dev, dst_dev in PLACES:
        offs, nt, ng = run_index(stream(name), src_dev, dst_dev)
        assert (nt, ng) == (len(want) - 1, want_runs), (name, src_dev, dst_dev, nt, ng)
        assert np.array_equal(offs[:nt + 1], want), (name, src_dev, dst_dev)
        assert np.all(offs[nt + 1:] == -7), (name, src_dev, dst_dev)     # nothing written behind offsets[nt]


@pytest.mark.parametrize("nt", CHAIN_LENGTHS)
def test_chain_lengths_around_every_doubling_round(nt):
    assert_index("chain of %d" % nt)


@pytest.mark.parametrize("name", ["200 exons among 2", "5000 exons among 2", "5000 exons first", "200 exons last"])
def test_long_records_among_short_ones(name):
    assert_index(name)


@pytest.mark.parametrize("name", DECOYS)
def test_decoys_leave_the_true_chain_only(name):
    assert_index(name)


@pytest.mark.parametrize("name", ["golden %d" % i for i in range(len(GOLDEN))] + sorted(EDGE_STREAMS) + ["equal and large graph ids"])
def test_streams_the_other_tests_use(name):
    assert_index(name)
    if name == "equal and large graph ids":
        assert expected(name)[1] == 3


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_refused_streams(name):
    w, why = MALFORMED[name]
    for src_dev, dst_dev in PLACES:
        with pytest.raises(A.DecompError) as e:
            run_index(w, src_dev, dst_dev)
        assert e.value.code == ERR_INVALID, (name, src_dev, dst_dev)
        assert ("ascending" in str(e.value)) == (why == "descending") and ("malformed" in str(e.value)) == (why != "descending"), (name, str(e.value))


@pytest.mark.parametrize("name", ["chain of 257", "200 exons among 2"])
def test_capacity_one_entry_too_few(name):
    want, want_runs = expected(name); nt = len(want) - 1
    for src_dev, dst_dev in PLACES:
        with pytest.raises(A.DecompError) as e:
            run_index(stream(name), src_dev, dst_dev, capacity=nt)
        assert e.value.code == ERR_INVALID and e.value.counts == (nt, want_runs), (name, src_dev, dst_dev, e.value.counts)
        offs, got_nt, ng = run_index(stream(name), src_dev, dst_dev, capacity=nt + 1)       # exactly enough
        assert (got_nt, ng) == (nt, want_runs) and np.array_equal(offs, want)
    import ctypes as C
    w = stream(name); a = C.c_int64(); b = C.c_int64()                  # counts only
    assert A.load_library().ald_tset_index_stream(0, C.c_void_p(w.ctypes.data), C.c_int64(w.size), None, C.c_int64(0), C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (nt, want_runs)
