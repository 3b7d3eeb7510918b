"""The exchange by bucket owner, CPU tier.  A transcript_set is a map from transcript::get_intron_chain_hashing to a bucket and
transcript_set::add only ever touches one bucket at a time, so rank hash % W can own a bucket outright.  Checked here, without a GPU:
ald_transcript_bucket against the hash the reference itself printed for all 908 golden items (tests/golden/ref_tset.json + the two cases of
make_golden_dev_tset), that no owner is vacuous for W = 2, 3, 8, and the PREMISE on the reference's own answers -- every golden case split
by owner, fed to W host sinks, interleaved by hash, equals the golden items exactly.  split_model is the numpy model of the split that
tests/test_owner_split_gpu.py holds the kernels to."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import aletsch_amd as A
from test_dev_tset_cpu import as_groups, check, mk

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = [(c["groups"], c["items"]) for c in json.load(open(os.path.join(HERE, "golden", "ref_tset.json")))] + mk.load()
WORLDS = (2, 3, 8)
HDR = 12                     # words in front of a transcript's exons in a transcript stream
M64 = (1 << 64) - 1
ENTRY_POINTS = ["ald_transcript_bucket", "ald_batch_device_transcript_streams_by_owner", "ald_tset_split_stream", "ald_comm_exchange_streams", "ald_comm_gather_sets"]


def bucket_of(x):
    """transcript::get_intron_chain_hashing over the flat exon words l0 r0 l1 r1 ..., written out independently of the library: no exon
    -> 0; one exon -> (l + r) / 10000 + 1 in int32 arithmetic (C division truncates); else hash_combine over the inner words, 31 bits + 1"""
    x = [int(v) for v in x]
    if len(x) < 2:
        return 0
    if len(x) == 2:
        s = (x[0] + x[1] + (1 << 31)) % (1 << 32) - (1 << 31)
        q = abs(s) // 10000 * (1 if s >= 0 else -1)
        return (q + 1) & M64
    h = len(x) - 2
    for v in x[1:-1]:
        h ^= ((v & M64) + 0x9e3779b9 + ((h << 6) & M64) + (h >> 2)) & M64
    return (h & 0x7FFFFFFF) + 1


def walk(words):
    """[(first word, words)] of every transcript of a stream"""
    out = []; o = 0
    while o < len(words):
        n = HDR + 2 * int(words[o + 5]); out.append((o, n)); o += n
    assert o == len(words)
    return out


def split_model(words, world):
    """the split, in numpy: a stable partition of the stream's transcripts by bucket % world -> (words, offsets[world + 1], order), order
    = for every transcript of the output its ordinal in the input"""
    words = np.ascontiguousarray(words, np.uint32)
    recs = walk(words)
    owner = [bucket_of(words[o + HDR:o + n].view(np.int32)) % world for o, n in recs]
    order = [i for r in range(world) for i in range(len(recs)) if owner[i] == r]
    offsets = np.zeros(world + 1, np.int64)
    for i in range(len(recs)):
        offsets[owner[i] + 1] += recs[i][1]
    out = np.concatenate([words[recs[i][0]:recs[i][0] + recs[i][1]] for i in order]) if order else np.zeros(0, np.uint32)
    return out, np.cumsum(offsets), order


def interleave(parts):
    """the items of W disjoint sets in the reference's iteration order: ascending hash; a bucket lives wholly in one part, so a stable sort
    of the concatenation keeps its inner order"""
    return sorted((x for p in parts for x in p), key=lambda x: x["hash"])


def test_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "aletsch_decomp.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", A.library_path()], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ald_\w+)", syms))
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in exported, name


def test_bucket_equals_the_reference_hash_of_every_golden_item():
    items = [x for _, it in GOLDEN for x in it]
    assert len(GOLDEN) == 8 and len(items) == 908 and sum(len(x["exons"]) == 1 for x in items) == 368
    for x in items:
        assert A.transcript_bucket(x["exons"]) == x["hash"] == bucket_of([v for e in x["exons"] for v in e]), x
    assert A.transcript_bucket([]) == 0
    # one exon: int32 arithmetic, C division (negative sums truncate toward zero, then widen to size_t)
    assert A.transcript_bucket([(-30000, 5000)]) == bucket_of([-30000, 5000]) == M64          # -25000 / 10000 = -2 (floor would give -3), + 1, as size_t
    assert A.transcript_bucket([(2000000000, 2000000000)]) == bucket_of([2000000000, 2000000000])
    import ctypes as C
    assert A.load_library().ald_transcript_bucket(None, 1, C.byref(C.c_uint64())) == -1
    assert A.load_library().ald_transcript_bucket(None, -1, C.byref(C.c_uint64())) == -1


def test_no_owner_is_vacuous():
    """the census of the issue: at least 20 items, 20 single-exon items and 20 items that merged (count > 1) per owner, W in {2, 3, 8}"""
    items = [x for _, it in GOLDEN for x in it]
    for W in WORLDS:
        for r in range(W):
            mine = [x for x in items if x["hash"] % W == r]
            assert len(mine) >= 20 and sum(len(x["exons"]) == 1 for x in mine) >= 20 and sum(x["count"] > 1 for x in mine) >= 20, (W, r)


def groups_of_owner(groups, world, r):
    """the groups (one per graph) with only the transcripts of the buckets owner r holds; a graph keeps its place and its sample id"""
    return [(sid, [t for t in ts if bucket_of([v for e in t[6] for v in e]) % world == r]) for sid, ts in groups]


@pytest.mark.parametrize("i", range(len(GOLDEN)))
def test_premise_owner_sinks_interleaved_equal_the_reference(i):
    groups, items = GOLDEN[i]; groups = as_groups(groups)
    for W in WORLDS:
        parts = []
        for r in range(W):
            s = A.TranscriptSink(0.8); s.add_groups(groups_of_owner(groups, W, r))
            parts.append(s.items()); s.close()
            assert all(x["hash"] % W == r for x in parts[-1])
        check(interleave(parts), items)


def test_model_is_a_stable_partition():
    from test_dev_tset_gpu import stream_of
    words, _, _ = stream_of(as_groups(GOLDEN[0][0]), 0)
    recs = walk(words)
    for W in (1, 2, 3, 8, 64):
        out, offs, order = split_model(words, W)
        assert sorted(order) == list(range(len(recs))) and offs[0] == 0 and offs[W] == len(words) == len(out)
        for r in range(W):
            seg = walk(out[offs[r]:offs[r + 1]])
            assert all(bucket_of(out[offs[r] + o + HDR:offs[r] + o + n].view(np.int32)) % W == r for o, n in seg)
        starts = np.cumsum([0] + [recs[i][1] for i in order])
        for r in range(W):                                           # inside an owner the ordinals ascend: the original order is kept
            mine = [i for k, i in enumerate(order) if offs[r] <= starts[k] < offs[r + 1]]
            assert mine == sorted(mine)
        if W == 1:
            assert np.array_equal(out, words)
