"""GPU tier: the results of a batch leave through a download stream of their own (ald_batch::dl_stream, ALD_DOWNLOAD_STREAM) while the
NEXT batch's kernel is already running.  What one stream ordered for free now rests on host waits, so every case drives batch objects in
the order of bench.py's main thread -- prev.sync(); cur.run(); prev.download() -- and asks each download for exactly what a serial
add / upload / run / download of the same graphs gave.

Four batch objects hold four DIFFERENT seeded sets (3000 graphs, V in 8..64, E = 4V, seeds 1..4): a download that read another batch's
buffers, or a buffer of an earlier step, cannot pass.  WHERE a record lies in the pool differs between two runs of the same build (the
wave that bumps the pool pointer first gets the lower offset), so results are compared through the index the kernel wrote, as
tests/test_compact_input_gpu.py does: record (g, p) word for word, plus status, path counts, iteration counts and the totals.

1. bench order, 8 steps; again with a fifth batch of 20 000 x 64v/256e as every second `cur` (a kernel of several milliseconds,
   certainly in flight while `prev` downloads).
2. the same rotation in a child process with ALD_DEBUG_UNDERCLASS=1 (capacity retry passes are launched from inside the download,
   beside the next kernel) and in one with ALD_DEBUG_POOL_WORDS small (the pool grows and the batch runs again from inside it).
3. finish() then download(), and finish() then device_transcript_stream(), each with the next kernel in flight.
4. ALD_DOWNLOAD_STREAM=0 / 1 / 2, one child process each: the same answers, and the same as this process got.

No case asserts a time.  The child processes are fresh interpreters running this file as a script."""
import hashlib
import os
import subprocess
import sys

if __name__ == "__main__":                                   # a child process: what tests/conftest.py does for the suite
    import torch  # noqa: F401  (its HIP runtime has to be the first one the process loads)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]

import numpy as np
import pytest

import aletsch_amd as A
from aletsch_amd.distributed import REC_HDR_WORDS, _device_words

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3, 4)
STEPS = 8
POOL_WORDS = 100000          # ALD_DEBUG_POOL_WORDS of case 2: a set needs several times that (asserted), so its first run finds the pool full


def small_set(seed):
    return A.synth(seed=seed, n_graphs=3000, v_min=8, v_max=64, edges_per_vertex=4)


def big_set():
    return A.synth(seed=1002, n_graphs=20000, v_min=64, v_max=64, fixed_edges=256)


def answer(b):
    """what a downloaded batch holds, free of pool placement: status / path / iteration counts, every record the index names in
    (graph, path) order as one word array + the records' lengths, and the totals (pool words in use, index entries)"""
    st, npth, nit = b.status_arrays()
    raw = b.raw_records(); idx, gf = b.result_index()
    cnt = np.where((st == 0) | (st == 1), npth, 0).astype(np.int64)
    first = np.repeat(gf, cnt); begin = np.cumsum(cnt) - cnt
    at = idx[first + (np.arange(int(cnt.sum())) - np.repeat(begin, cnt))].astype(np.int64)        # pool offset of record (g, p)
    ln = (REC_HDR_WORDS + raw[at + 2].astype(np.int64) + raw[at + 14].astype(np.int64) + 1) & ~1
    rb = np.cumsum(ln) - ln
    words = raw[np.repeat(at, ln) + (np.arange(int(ln.sum())) - np.repeat(rb, ln))]
    return dict(status=st.copy(), npaths=npth.copy(), iters=nit.copy(), iterations=b.iterations().copy(), lengths=ln, words=words,
                totals=np.array([raw.size, idx.size], np.int64))


def same(got, want, what):
    for k in ("status", "npaths", "iters", "iterations", "totals", "lengths", "words"):
        assert np.array_equal(got[k], want[k]), (what, k)


def digest(ans, keys=("status", "npaths", "iters", "iterations", "totals", "lengths", "words")):
    h = hashlib.sha256()
    for k in keys:
        h.update(np.ascontiguousarray(ans[k]).tobytes())
    return h.hexdigest()


def digest_shape(ans):
    """what a run with capacity retries shares with a plain run: status, path counts and the length of every record (a record carries the
    number of the pass that wrote it, and the abandoned attempts of a retried graph stay in the pool: words and totals differ)"""
    return digest(ans, ("status", "npaths", "lengths"))


def stream_words(b):
    import torch
    ptr, n = b.device_transcript_stream()
    return _device_words(ptr, n, torch.device("cuda", 0)).cpu().numpy().view(np.uint32).copy() if n else np.zeros(0, np.uint32)


def serial(pg):
    """a batch object that has gone through add / upload / run / download once, and its answer: the reference"""
    b = A.DecompBatch(0)
    b.add(pg); b.upload(); b.run(); b.download()
    return b, answer(b)


def rotate(batches, wants, order, end="download", reupload=False, after=None):
    """bench.py's main thread over resident batches: `order` names the batch of every step.  end: how `prev` ends under cur's kernel
    (download | finish_download | finish_stream: the latter compares the device-built transcript stream with want["stream"]);
    reupload: every batch is uploaded again before it runs (its pool starts small again under ALD_DEBUG_POOL_WORDS);
    after(batch): extra check on a batch that has just been downloaded."""
    def finish(i):
        b, want = batches[i], wants[i]
        if end == "finish_stream":
            b.finish()
            assert np.array_equal(stream_words(b), want["stream"]), ("device stream", i)
            for x, k in zip(b.status_arrays(), ("status", "npaths", "iters")):
                assert np.array_equal(x, want[k]), (end, i, k)
            return
        if end == "finish_download":
            b.finish()
        b.download()
        same(answer(b), want, (end, i))
        if after:
            after(b)
    prev = None
    for i in order:
        cur = batches[i]
        if reupload:
            cur.upload()
        if prev is not None:
            batches[prev].sync()
        cur.run()
        if prev is not None:
            finish(prev)
        prev = i
    finish(prev)


ORDER = [k % 4 for k in range(STEPS)]
ORDER_BIG = [4 if k % 2 else (k // 2) % 4 for k in range(STEPS)]          # the fifth batch is every second `cur`


@pytest.fixture(scope="module")
def ref():
    """four batch objects, each run serially once over its own set: the objects (resident from here on) and their answers"""
    made = [serial(small_set(s)) for s in SEEDS]
    batches = [m[0] for m in made]; wants = [m[1] for m in made]
    for w in wants:
        assert (w["status"] == 0).all() and w["lengths"].size > 3000
    assert len({digest(w) for w in wants}) == 4              # the sets differ
    yield batches, wants
    for b in batches:
        b.close()


def test_bench_order(ref):
    batches, wants = ref
    rotate(batches, wants, ORDER)


def test_bench_order_beside_a_long_kernel(ref):
    batches, wants = ref
    big, want_big = serial(big_set())
    try:                                                     # (a fifth of the bench batch: its kernel runs for several milliseconds)
        rotate(batches + [big], wants + [want_big], ORDER_BIG)
    finally:
        big.close()


@pytest.mark.parametrize("end", ["finish_download", "finish_stream"])
def test_finish_first(ref, end):
    batches, wants = ref
    if end == "finish_stream":
        wants = [dict(w, stream=stream_words(b)) for b, w in zip(batches, wants)]      # of the downloaded batches, as the fixture or an earlier rotation left them
        assert all(w["stream"].size > 0 for w in wants)
        rotate(batches, wants, ORDER, end)
        for b, w in zip(batches, wants):                     # finished only: the records are still to be had
            b.download(); same(answer(b), w, "download after the stream")
    else:
        rotate(batches, wants, ORDER, end)


# ---- child processes: the modes are read when the library is loaded / a batch is created ----
def child(mode):
    made = [serial(small_set(s)) for s in SEEDS]
    batches = [m[0] for m in made]; wants = [m[1] for m in made]
    after = None
    if mode == "pool":
        for w in wants:                                      # the serial run itself outgrew the pool it started with
            assert w["totals"][0] > POOL_WORDS and (w["status"] == 0).all(), w["totals"]
        def after(b):
            assert b.raw_records().size > POOL_WORDS
    rotate(batches, wants, ORDER, reupload=(mode == "pool"), after=after)
    for w in wants:
        print("answer", digest(w), digest_shape(w))
    for b in batches:
        b.close()


def run_child(mode, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("ALD_DOWNLOAD_STREAM", "ALD_DEBUG_UNDERCLASS", "ALD_DEBUG_POOL_WORDS", "ALD_DEBUG_RETRY")}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=240, env=e)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("answer ")]
    return [ln[1] for ln in lines], [ln[2] for ln in lines], r.stderr


def test_capacity_retries_beside_the_next_kernel(ref):
    _, shapes, err = run_child("plain", ALD_DEBUG_UNDERCLASS="1", ALD_DEBUG_RETRY="1")
    # every set runs three times in the child (once serially, twice in the rotation) and a run's overflows do not depend on timing
    k = err.count("overflowed class")
    assert k > 0 and k % 3 == 0, (k, err[-2000:])
    assert shapes == [digest_shape(w) for w in ref[1]]       # (the child itself compared every download with its serial run in full)


def test_pool_regrow_beside_the_next_kernel(ref):
    got, _, _ = run_child("pool", ALD_DEBUG_POOL_WORDS=str(POOL_WORDS))
    assert got == [digest(w) for w in ref[1]]                # a batch that ran again from pass 0 gives the plain answer, totals included


@pytest.mark.parametrize("routing", ["0", "1", "2"])
def test_stream_routings_agree(ref, routing):
    got, _, _ = run_child("plain", ALD_DOWNLOAD_STREAM=routing)
    assert got == [digest(w) for w in ref[1]]


if __name__ == "__main__":
    child(sys.argv[1])
