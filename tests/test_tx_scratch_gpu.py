"""The batch-side entry points that share the reduction's scratch, interleaved on ONE batch: the reduction, the device transcript stream, the
owner split and the fold into a resident set all take buffers of the batch's front-end scratch (sample ids, hipCUB storage, a pinned counter),
so every one of them has to leave the others' results alone whatever ran before it.  Each result of the interleaved sequence must equal,
word for word and FP64 by bits, the result of the same single call on a fresh batch of the same graphs -- forwards, backwards, and on a
batch that ald_batch_finish ended (where the reduction refuses, as it does on the fresh batch)."""
import functools
import struct

import numpy as np
import pytest

import aletsch_amd as A
from aletsch_amd.distributed import _device_words

pytestmark = pytest.mark.gpu
HDR = 12
WORLD = 3


@functools.lru_cache(maxsize=None)
def graphs():
    return A.synth(seed=49, n_graphs=300, v_min=6, v_max=40, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=2, strand_mode=1)


@functools.lru_cache(maxsize=None)
def sample_ids():
    rng = np.random.default_rng(49); n = graphs().n
    sid_a = rng.integers(-1, 8, n).astype(np.int32); sid_b = rng.integers(-1, 8, n).astype(np.int32)
    assert sid_a.min() >= -1 and sid_a.max() <= 7 and sid_b.min() >= -1 and sid_b.max() <= 7 and not np.array_equal(sid_a, sid_b)
    return sid_a, sid_b


def bits(x):
    """a result in a form == compares exactly: FP64 by its bits, arrays by their bytes"""
    if isinstance(x, float):
        return struct.unpack("<Q", struct.pack("<d", x))[0]
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return {k: bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [bits(v) for v in x]
    return x


def to_host(ptr, n_words):
    """the words of a device result, copied before the next call may overwrite them"""
    import torch
    if n_words == 0:
        return np.zeros(0, np.uint32)
    return _device_words(ptr, n_words, torch.device("cuda", 0)).cpu().numpy().view(np.uint32).copy()


def stream(b, sid, skip):
    return to_host(*b.device_transcript_stream(sid, skip))


def by_owner(b, sid):
    p, offs = b.device_transcript_streams_by_owner(WORLD, sid)
    return to_host(p, int(offs[WORLD])), offs


def into_set(b, sid):
    with A.DeviceTranscriptSet(0, 0.8) as ds:
        ds.add_batch(b, sid)
        return ds.items()


def calls():
    sid_a, sid_b = sample_ids()
    return [("reduce a", lambda b: b.reduce_transcripts(sid_a)[0]),
            ("by owner b", lambda b: by_owner(b, sid_b)),
            ("stream a", lambda b: stream(b, sid_a, False)),
            ("reduce b, no single-exon", lambda b: b.reduce_transcripts(sid_b, skip_single_exon=True)[0]),
            ("stream b, no single-exon", lambda b: stream(b, sid_b, True)),
            ("resident set a", lambda b: into_set(b, sid_a))]


def result_of(call, b):
    try:
        return bits(call(b))
    except A.DecompError as e:                               # (the reduction on a batch that was only finished)
        return ("error", e.code, str(e))


def ended(end):
    b = A.DecompBatch(0)
    b.add(graphs()); b.upload(); b.run(); getattr(b, end)()
    return b


@functools.lru_cache(maxsize=None)
def single(end):
    """every call alone on a fresh batch: computed once, never changed"""
    out = {}
    for name, call in calls():
        with ended(end) as b:
            out[name] = result_of(call, b)
    return out


def test_neither_branch_is_vacuous():
    w = single("download")["stream a"][2]
    w = np.frombuffer(w, np.uint32)
    n_paths = 0; n_single = 0; o = 0
    while o < w.size:
        ne = int(w[o + 5]); n_paths += 1; n_single += ne <= 1; o += HDR + 2 * ne
    print(f"paths {n_paths}, single-exon transcripts {n_single}")
    assert n_paths > 300 and n_single >= 1
    assert single("download")["stream b, no single-exon"] != single("download")["stream a"]
    assert single("finish")["reduce a"][0] == "error" and single("download")["reduce a"][0] != "error"


@pytest.mark.parametrize("end", ["download", "finish"])
@pytest.mark.parametrize("order", ["forwards", "backwards"])
def test_interleaved_calls_equal_single_calls(end, order):
    want = single(end)
    seq = calls() if order == "forwards" else calls()[::-1]
    with ended(end) as b:
        for name, call in seq:
            got = result_of(call, b)
            assert got == want[name], f"{name} ({order}, after {end}) differs from the same call on a fresh batch"
