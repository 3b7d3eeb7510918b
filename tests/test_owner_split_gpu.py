"""The exchange by bucket owner on the GPU (aletsch_amd/csrc/tset_partition.hip, comm_rccl.cpp): the split kernels against the numpy model of
tests/test_owner_split_cpu.py word for word, the batch form against the model applied to the unsplit stream, the reference's golden cases
through W owner sets, and the whole step -- split, all-to-all exchange, fold, collection of the sets -- with the ranks as threads over the
mock RCCL (tests/host_adapter/exchange_ranks_test.cc).  Every comparison is exact."""
import functools
import os
import subprocess

import numpy as np
import pytest

import aletsch_amd as A
from test_dev_tset_cpu import as_groups, check
from test_dev_tset_gpu import stream_of
from test_owner_split_cpu import GOLDEN, HDR, ROOT, WORLDS, interleave, split_model, walk

pytestmark = pytest.mark.gpu
ERR_INVALID = -1


@functools.lru_cache(maxsize=None)
def golden_stream(i):
    return stream_of(as_groups(GOLDEN[i][0]), 0)


def one(graph, path, exons, sid=-1, strand="+", weight=1.5):
    h = np.zeros(HDR, np.uint32)
    h[0] = graph; h[1] = path; h[2] = np.uint32(sid & 0xFFFFFFFF); h[3] = ord(strand); h[4] = 1; h[5] = len(exons)
    h[6:8] = np.array([weight]).view(np.uint32); h[8:10] = np.array([0.5]).view(np.uint32); h[10:12] = np.array([2.0]).view(np.uint32)
    return np.concatenate([h, np.array(exons, np.int32).reshape(-1).view(np.uint32)])


def chain(n, start):
    return [(start + 100 * k, start + 100 * k + 60) for k in range(n)]


EDGE_STREAMS = {
    "empty": np.zeros(0, np.uint32),
    "one transcript": one(3, 0, chain(4, 1000)),
    "single-exon only": np.concatenate([one(g, p, [(10000 * (3 * g + p), 10000 * (3 * g + p) + 700)]) for g in range(40) for p in range(3)]),
    # a 16-lane group that loops 26 times beside groups that loop once
    "200 exons among 2": np.concatenate([one(g, 0, chain(2, 5000 * g)) for g in range(20)] + [one(20, 0, chain(200, 77))] + [one(g, 0, chain(2, 5000 * g)) for g in range(21, 41)]),
    "zero exons": np.concatenate([one(0, 0, chain(3, 10)), one(0, 1, []), one(1, 0, chain(2, 900)), one(2, 0, [])]),
}


def run_split(words, world, src_dev=False, dst_dev=False):
    """ald_tset_split_stream with source / destination in host or device memory -> (words, offsets)"""
    import torch
    words = np.ascontiguousarray(words, np.uint32); n = words.size
    offs = np.full(max(world, 0) + 1, -7, np.int64)
    keep = []
    if src_dev and n:
        t = torch.from_numpy(words.view(np.int32).copy()).cuda(); keep.append(t); src = t.data_ptr()
    else:
        src = words.ctypes.data
    out = np.zeros(max(n, 1), np.uint32)
    if dst_dev and n:
        d = torch.zeros(n, dtype=torch.int32, device="cuda"); torch.cuda.synchronize(); dst = d.data_ptr()
    else:
        dst = out.ctypes.data
    A.split_stream_into(src, n, world, dst, offs)
    if dst_dev and n:
        out = d.cpu().numpy().view(np.uint32)
    return out[:n], offs


def assert_split(words, world, **where):
    got, offs = run_split(words, world, **where)
    want, woffs, _ = split_model(words, world)
    assert np.array_equal(offs, woffs), (world, where, offs, woffs)
    assert np.array_equal(got, want), (world, where)


@pytest.mark.parametrize("world", (1, 2, 3, 8, 64))
def test_kernel_matches_the_model_word_for_word(world):
    for i in range(len(GOLDEN)):
        assert_split(golden_stream(i)[0], world)
    big = golden_stream(len(GOLDEN) - 2)[0]                       # 2000 groups: several blocks of every kernel
    assert len(walk(big)) > 2000
    for src_dev in (False, True):
        for dst_dev in (False, True):
            assert_split(big, world, src_dev=src_dev, dst_dev=dst_dev)
    for name, w in EDGE_STREAMS.items():
        for dev in (False, True):
            assert_split(w, world, src_dev=dev, dst_dev=dev)
    if world == 1:
        assert np.array_equal(run_split(big, 1)[0], big)
    # refused: a world outside 1..64, a truncated stream, a stream whose graphs descend
    w = EDGE_STREAMS["200 exons among 2"]
    for bad_world in (0, 65):
        with pytest.raises(A.DecompError) as e:
            run_split(w, bad_world)
        assert e.value.code == ERR_INVALID
    for bad in (w[:-1], w[:HDR - 2], np.concatenate([one(5, 0, chain(2, 10)), one(4, 0, chain(2, 10))])):
        for dev in (False, True):
            with pytest.raises(A.DecompError) as e:
                run_split(bad, world, src_dev=dev)
            assert e.value.code == ERR_INVALID


def device_words(ptr, n):
    import torch
    from aletsch_amd.distributed import _device_words
    if n == 0:
        return np.zeros(0, np.uint32)
    return _device_words(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(np.uint32).copy()


def test_batch_form_equals_the_model_on_the_unsplit_stream():
    pg = A.synth(seed=77, n_graphs=300, v_min=8, v_max=40, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)
    sid = (np.arange(pg.n) % 7 - 1).astype(np.int32)
    with A.DecompBatch(0) as bd, A.DecompBatch(0) as bf:
        bd.add(pg); bd.upload(); bd.run(); bd.download()
        bf.add(pg); bf.upload(); bf.run(); bf.finish()
        for skip in (False, True):
            for s in (sid, None):
                stream = bd.transcript_stream(s, skip)
                assert len(walk(stream)) > 600
                for W in WORLDS:
                    want, woffs, _ = split_model(stream, W)
                    for b in (bd, bf):
                        ptr, offs = b.device_transcript_streams_by_owner(W, s, skip)
                        assert np.array_equal(offs, woffs), (W, skip)
                        assert np.array_equal(device_words(ptr, int(offs[W])), want), (W, skip)
                for b in (bd, bf):
                    ptr, offs = b.device_transcript_streams_by_owner(1, s, skip)
                    p1, n1 = b.device_transcript_stream(s, skip)
                    assert list(offs) == [0, n1] and np.array_equal(device_words(ptr, n1), device_words(p1, n1)) and np.array_equal(device_words(p1, n1), stream)
        full = bd.transcript_stream(None, False)
        assert any(int(full[o + 5]) == 1 for o, n in walk(full))     # single-exon transcripts took part
        for bad_world in (0, 65):
            with pytest.raises(A.DecompError) as e:
                bd.device_transcript_streams_by_owner(bad_world)
            assert e.value.code == ERR_INVALID
    with A.DecompBatch(0) as b:                                     # before the run has ended: ALD_ERR_STATE
        b.add(pg); b.upload(); b.run(); b.sync()
        with pytest.raises(A.DecompError) as e:
            b.device_transcript_streams_by_owner(2)
        assert e.value.code == -4


@pytest.mark.parametrize("i", range(len(GOLDEN)))
def test_golden_cases_through_owner_sets(i):
    """every golden case, W in {2, 3, 8}, its groups cut into 1 and into 3 consecutive source shards: owner r's resident set takes segment
    r of every shard in shard order with that shard's graph offset; the W snapshots interleaved by hash are the reference's items"""
    groups, items = GOLDEN[i]; groups = as_groups(groups)
    for n_shards in (1, 3):
        cuts = [len(groups) * k // n_shards for k in range(n_shards + 1)]
        shards = [(a, stream_of(groups[a:b], 0)) for a, b in zip(cuts[:-1], cuts[1:])]
        for W in WORLDS:
            sets = [A.DeviceTranscriptSet(0, 0.8) for _ in range(W)]
            try:
                for first, (words, cov, tid) in shards:
                    where = {(int(words[o]), int(words[o + 1])): k for k, (o, n) in enumerate(walk(words))}
                    out, offs = A.split_stream(words, W)
                    for r in range(W):
                        seg = out[offs[r]:offs[r + 1]]
                        pick = [where[(int(seg[o]), int(seg[o + 1]))] for o, n in walk(seg)]     # which transcripts the kernel put here: their coverage / id travel along
                        sets[r].add_stream(seg, coverage=cov[pick], tid=tid[pick], graph_offset=first)
                parts = [s.items() for s in sets]
            finally:
                for s in sets:
                    s.close()
            for r in range(W):
                assert all(x["hash"] % W == r for x in parts[r])
            check(interleave(parts), items)


def test_exchange_with_several_ranks_on_one_gpu():
    """split -> ald_comm_exchange_streams -> fold -> ald_comm_gather_sets with W = 2, 3 and 8 ranks as threads over the mock RCCL: rank 0's
    flat equals the host set fed all shards unsplit; then a refused ncclSend (every rank returns an error, out of group mode) and a set
    that holds a foreign bucket (ALD_ERR_INVALID on all ranks)"""
    bld = os.path.join(ROOT, "tests", "_build"); os.makedirs(bld, exist_ok=True)
    lib = os.path.join(ROOT, "aletsch_amd", "lib"); mock = os.path.join(bld, "libmock_rccl.so"); exe = os.path.join(bld, "exchange_ranks_test")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "-o", mock, os.path.join(ROOT, "tests", "host_adapter", "mock_rccl.cc")], check=True)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "host_adapter", "exchange_ranks_test.cc"), "-o", exe, "-L" + lib, "-laletsch_decomp", "-Wl,-rpath," + lib,
                    "-L/opt/rocm/lib", "-lamdhip64", "-ldl", "-pthread"], check=True)
    env = dict(os.environ, ALD_RCCL_LIB=mock); env.pop("ALD_MOCK_RCCL_FAIL_SEND", None)
    for world in ("2", "3", "8"):
        r = subprocess.run([exe, world], capture_output=True, text=True, timeout=90, env=env)
        assert r.returncode == 0 and "EXCHANGE_RANKS_OK world=" + world + " items=" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
    for world in ("2", "3"):
        r = subprocess.run([exe, world, "fail"], capture_output=True, text=True, timeout=90, env=dict(env, ALD_MOCK_RCCL_FAIL_SEND="1"))
        assert r.returncode == 0 and "injected send failure handled on every rank" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
        r = subprocess.run([exe, world, "foreign"], capture_output=True, text=True, timeout=90, env=env)
        assert r.returncode == 0 and "foreign bucket refused on every rank" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
