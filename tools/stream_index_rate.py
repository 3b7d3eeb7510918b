# What it costs the owner of a bucket range to fold a segment that lies in HBM (ald_tset_dev_add_stream on a device pointer), on the bench
# shape: one finished 100 000 x 64v/256e batch, its device stream (~153 MB, ~1.9 M transcripts) and owner 0's sub-stream at W = 8.
# For each of the two: fold into an EMPTY set ("cold"), then fold the same words again into the now warm set ("warm"), five times after one
# discarded run; per fold last_call_ms (wall, the whole call) and last_device_ms (HIP events) of ald_tset_dev_stats and, where the library
# has them, index_ms and bytes_to_host of ald_tset_dev_stream_stats; then ald_tset_split_stream device -> device on the full stream (wall).
# Run it once per library to compare two builds: ALETSCH_DECOMP_LIB=<older libaletsch_decomp.so> prints the first two figures only.
# Prints one JSON line.
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import aletsch_amd as A
from aletsch_amd.distributed import _device_words

N = int(os.environ.get("N", "100000")); W = int(os.environ.get("W", "8")); RUNS = 5
lib = A.load_library()
HAS_STATS = hasattr(lib, "ald_tset_dev_stream_stats")
dev = torch.device("cuda", 0)


def fold_twice(t):
    out = {}
    with A.DeviceTranscriptSet(0, 0.8) as ds:
        for phase in ("cold", "warm"):
            torch.cuda.synchronize()
            ds.add_stream_ptr(t.data_ptr(), t.numel())
            st = ds.stats()
            r = dict(last_call_ms=round(st["call_ms"], 3), last_device_ms=round(st["device_ms"], 3))
            if HAS_STATS:
                ss = ds.stream_stats()
                r.update(index_ms=round(ss["index_ms"], 3), bytes_to_host=ss["bytes_to_host"], words_to_host=ss["words_to_host"], n_transcripts=ss["n_transcripts"])
            out[phase] = r
        out["items"] = ds.size()[0]
    return out


pg = A.synth(seed=1002, n_graphs=N, v_min=64, v_max=64, fixed_edges=256)
with A.DecompBatch(0) as b:
    b.add(pg); b.upload(); b.run(); b.finish()
    p, n_words = b.device_transcript_stream(None, True)
    full = _device_words(p, n_words, dev).clone()
    p, offs = b.device_transcript_streams_by_owner(W, None, True)
    seg = _device_words(p, int(offs[1]), dev).clone()
torch.cuda.synchronize()
res = dict(tool="stream_index_rate", library=os.path.basename(os.path.dirname(A.library_path())) + "/" + os.path.basename(A.library_path()), has_stream_stats=HAS_STATS,
           n_graphs=N, world=W, full_words=int(n_words), full_mb=round(4 * n_words / 1e6, 1), segment_words=int(offs[1]), segment_mb=round(4 * int(offs[1]) / 1e6, 1))
for name, t in (("full", full), ("segment", seg)):
    runs = [fold_twice(t) for _ in range(RUNS + 1)][1:]               # the first run is discarded
    res[name] = runs
    for phase in ("cold", "warm"):
        v = [r[phase]["last_call_ms"] for r in runs]
        res["%s_%s_call_ms_min_max" % (name, phase)] = [min(v), max(v)]
out = torch.empty_like(full); offs2 = np.zeros(W + 1, np.int64); split_ms = []
for _ in range(RUNS + 1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    A.split_stream_into(full.data_ptr(), full.numel(), W, out.data_ptr(), offs2)
    split_ms.append(round(1e3 * (time.perf_counter() - t0), 3))
assert int(offs2[W]) == n_words and int(offs2[1]) == int(offs[1])
res["split_full_dev_to_dev_ms"] = split_ms[1:]
print(json.dumps(res))
