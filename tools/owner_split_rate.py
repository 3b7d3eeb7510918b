# What the split by bucket owner costs next to the unsplit stream, on the bench shape (100 000 x 64v/256e, one finished batch, W = 8):
#   stream     ald_batch_device_transcript_stream              lengths, scan, fill
#   by_owner   ald_batch_device_transcript_streams_by_owner    owner + lengths, radix sort over 3 bits, scan, fill in owner order
# both in one process on the same batch, three runs each after one warm-up, timed with HIP events around the call (torch.cuda.Event on
# the current stream; both calls wait for their own stream before they return, so the events bracket all their device work and their host
# time).  Prints one JSON line: ms per run, transcripts, words, and the ratio of the medians.
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import aletsch_amd as A

N = int(os.environ.get("N", "100000")); W = int(os.environ.get("W", "8")); RUNS = 3


def timed(f):
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record(); out = f(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b), out


pg = A.synth(seed=1002, n_graphs=N, v_min=64, v_max=64, fixed_edges=256)
with A.DecompBatch(0) as b:
    b.add(pg); b.upload(); b.run(); b.finish()
    stream = lambda: b.device_transcript_stream(None, True)
    owners = lambda: b.device_transcript_streams_by_owner(W, None, True)
    stream(); owners()                                             # warm-up: buffers allocated, path table built
    t_stream = []; t_owner = []
    for _ in range(RUNS):
        ms, (_, n_words) = timed(stream); t_stream.append(ms)
        ms, (_, offs) = timed(owners); t_owner.append(ms)
    assert int(offs[W]) == n_words
print(json.dumps(dict(tool="owner_split_rate", n_graphs=N, world=W, words=int(n_words), mb=round(4 * n_words / 1e6, 1),
                      stream_ms=[round(x, 3) for x in t_stream], by_owner_ms=[round(x, 3) for x in t_owner],
                      words_per_owner=[int(x) for x in np.diff(offs)],
                      ratio_of_medians=round(float(np.median(t_owner) / np.median(t_stream)), 3))))
