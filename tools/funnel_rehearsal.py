#!/usr/bin/env python3
"""Rank 0's funnel at N > 1, rehearsed on ONE GPU: W ranks as threads of this process, RCCL replaced by tests/host_adapter/mock_rccl.cc
(ALD_RCCL_LIB; device-to-device copies behind the nccl* entry points), every rank holding the finished-transcript stream of ITS OWN
cfg4 shard (BASELINE.json configs[3]: 125 000 graphs of 64v / 256e, seed 1004 + rank) in device memory.

Per step every rank calls ald_comm_gather_begin; rank 0 then waits for stream r to land in pinned host memory (ald_comm_gather_wait(r))
and merges it (ald_tset_add_stream) while stream r + 1 is still being copied.  Printed: receive (mock: D2D) + D2H until everything has
landed, the merge per stream, the whole step, and the same with the next step's gather begun BEFORE the merge (the buffers exist twice).
What the rehearsal cannot show is the xGMI time of the real receive: 8 x ~180 MB over 7 links of ~50 GB/s is a few milliseconds.

    ALD_RCCL_LIB=tests/_build/libmock_rccl.so python tools/funnel_rehearsal.py [W=8] [graphs per rank=125000] [steps=3] [mode=funnel]

mode `owners`: the exchange by bucket owner instead of the funnel.  Per step every rank splits its stream by owner on the device
(ald_tset_split_stream, device to device), exchanges the sub-streams all to all (ald_comm_exchange_streams) and folds the W segments it
received, in rank order, into its OWN resident set (ald_tset_dev_add_stream); after the last step the sets go to rank 0
(ald_comm_gather_sets).  Printed per rank: the transcripts folded per step, the fold time, the share of all transcripts and of all items it
holds.  W ranks share one GPU and this host's cores here, so the fold times are upper bounds; what the run shows is the share.
"""
import ctypes as C, os, subprocess, sys, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = int(sys.argv[1]) if len(sys.argv) > 1 else 8
NG = int(sys.argv[2]) if len(sys.argv) > 2 else 125000
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
MODE = sys.argv[4] if len(sys.argv) > 4 else "funnel"
assert MODE in ("funnel", "owners"), MODE
mock = os.environ.get("ALD_RCCL_LIB")
if not mock:
    mock = os.path.join(ROOT, "tests", "_build", "libmock_rccl.so"); os.makedirs(os.path.dirname(mock), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-shared", "-fPIC", "-o", mock, os.path.join(ROOT, "tests", "host_adapter", "mock_rccl.cc")], check=True)
    os.environ["ALD_RCCL_LIB"] = mock
import numpy as np
import torch
import aletsch_amd as A
from aletsch_amd.distributed import _device_words
lib = A.load_library()
lib.ald_comm_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
lib.ald_comm_gather_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
lib.ald_comm_gather_wait.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(C.c_int32))]
lib.ald_comm_destroy.argtypes = [C.c_void_p]
lib.ald_tset_add_stream.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64]

# every rank's stream, built by its own decomposition run, parked in a device tensor of its own
dev = torch.device("cuda", 0); streams = []; t0 = time.perf_counter()
with A.DecompBatch(0) as b:
    for r in range(W):
        pg = A.synth(seed=1004 + r, n_graphs=NG, v_min=64, v_max=64, fixed_edges=256)
        b.clear(); b.add(pg); b.upload(); b.run(); b.download()
        ptr, n = b.device_transcript_stream(None, True)                     # single-exon transcripts left out, as the reference's default
        streams.append(_device_words(ptr, n, dev).clone())
torch.cuda.synchronize()
print(f"{W} shards of {NG} graphs decomposed in {time.perf_counter() - t0:.1f} s; stream sizes (MB): {[round(4 * s.numel() / 1e6, 1) for s in streams]}", flush=True)

uid = (C.c_uint8 * 128)(); assert lib.ald_comm_unique_id(uid) == 0, lib.ald_last_error()


def owners():
    lib.ald_comm_exchange_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(C.c_int32))]
    lib.ald_comm_gather_sets.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    bar = threading.Barrier(W); rep = [None] * W; err = []; total = {}

    def n_transcripts(words):                                    # the records of a stream, counted on the host
        w = words.cpu().numpy().view(np.uint32); n = 0; o = 0
        while o < w.size:
            o += 12 + 2 * int(w[o + 5]); n += 1
        return n

    def rank(r):
        try:
            comm = C.c_void_p(); assert lib.ald_comm_create(uid, W, r, 0, C.byref(comm)) == 0, lib.ald_last_error()
            src = streams[r]; split = torch.empty_like(src); offs = np.zeros(W + 1, np.int64); torch.cuda.synchronize()
            steps = []
            with A.DeviceTranscriptSet(0, 0.8) as ds:
                for k in range(STEPS):
                    bar.wait(); t0 = time.perf_counter()
                    A.split_stream_into(src.data_ptr(), src.numel(), W, split.data_ptr(), offs)
                    t1 = time.perf_counter()
                    words = C.c_void_p(); seg = C.POINTER(C.c_int64)(); goffs = C.POINTER(C.c_int32)()
                    assert lib.ald_comm_exchange_streams(comm, C.c_void_p(split.data_ptr()), C.c_void_p(offs.ctypes.data), C.c_int32(r * NG), C.byref(words), C.byref(seg), C.byref(goffs)) == 0, lib.ald_last_error()
                    t2 = time.perf_counter(); got = seg[W]
                    if k == 0:
                        total[r] = n_transcripts(_device_words(words.value, got, dev)) if got else 0; bar.wait(); t2 = time.perf_counter()
                    for q in range(W):
                        n = seg[q + 1] - seg[q]
                        if n:
                            assert lib.ald_tset_dev_add_stream(ds._h, C.c_void_p(words.value + 4 * seg[q]), C.c_int64(n), None, None, C.c_int32(goffs[q]), C.c_int64((k + 1) << 44), C.c_int32(0)) == 0, lib.ald_last_error()
                    t3 = time.perf_counter()
                    steps.append((t1 - t0, t2 - t1, t3 - t2, 4 * got / 1e6))
                bar.wait(); t0 = time.perf_counter()
                snap = C.c_void_p(); assert lib.ald_tset_dev_snapshot(ds._h, C.byref(snap)) == 0, lib.ald_last_error()
                items = C.c_int64(); assert lib.ald_tset_flat_size(snap, C.byref(items), None, None) == 0
                allf = C.c_void_p(); assert lib.ald_comm_gather_sets(comm, snap, C.byref(allf)) == 0, lib.ald_last_error()
                t1 = time.perf_counter(); merged = C.c_int64(0)
                if allf.value:
                    assert lib.ald_tset_flat_size(allf, C.byref(merged), None, None) == 0; lib.ald_tset_flat_free(allf)
                lib.ald_tset_flat_free(snap)
                rep[r] = (steps, items.value, merged.value, t1 - t0)
            bar.wait()
            assert lib.ald_comm_destroy(comm) == 0
        except BaseException as e:
            err.append(e)
            try: bar.abort()
            except Exception: pass

    ths = [threading.Thread(target=rank, args=(r,)) for r in range(W)]
    for t in ths: t.start()
    for t in ths: t.join()
    if err: raise err[0]
    all_tx = sum(total.values()); all_items = sum(x[1] for x in rep)
    for r in range(W):
        steps, items, merged, tg = rep[r]
        print(f"rank {r}: folds {total[r]} of {all_tx} transcripts per step (share {total[r] / all_tx:.4f}), {steps[0][3]:.0f} MB received | " +
              " | ".join(f"step {k}: split {1e3 * a:6.1f} ms, exchange {1e3 * b:6.1f} ms, fold {1e3 * c:7.1f} ms" for k, (a, b, c, _) in enumerate(steps)) +
              f" | holds {items} of {all_items} items (share {items / all_items:.4f})", flush=True)
    worst = max(max(c for _, _, c, _ in rep[r][0][1:] or rep[r][0]) for r in range(W))
    print(f"largest share of the transcripts folded by one rank: {max(total.values()) / all_tx:.4f} (1 / W = {1 / W:.4f}); largest share of the items held: {max(x[1] for x in rep) / all_items:.4f}")
    print(f"slowest fold of one rank after the first step: {1e3 * worst:.1f} ms for {W * NG} bundles of the step = {W * NG / worst / 1e6:.2f} M bundles/s with all {W} ranks on ONE GPU and one host")
    print(f"sets to rank 0 (snapshot + ald_comm_gather_sets, {rep[0][2]} items in the merged flat): {1e3 * rep[0][3]:.1f} ms, once per run")
    assert rep[0][2] == all_items
    print("OWNERS_OK")


if MODE == "owners":
    owners(); sys.exit(0)
sink = A.TranscriptSink(0.8)
bar = threading.Barrier(W); rep = {}; err = []

def rank(r):
    try:
        comm = C.c_void_p(); assert lib.ald_comm_create(uid, W, r, 0, C.byref(comm)) == 0, lib.ald_last_error()
        src = streams[r]
        for mode in ("serial", "overlapped"):
            for k in range(STEPS):
                bar.wait(); t_begin = time.perf_counter()
                assert lib.ald_comm_gather_begin(comm, C.c_void_p(src.data_ptr()), C.c_int64(src.numel()), C.c_int32(r * NG)) == 0, lib.ald_last_error()
                t_enq = time.perf_counter()
                allw = C.POINTER(C.c_uint32)(); offs = C.POINTER(C.c_int64)(); goffs = C.POINTER(C.c_int32)()
                if r != 0:
                    assert lib.ald_comm_gather_wait(comm, -1, C.byref(allw), C.byref(offs), C.byref(goffs)) == 0
                    continue
                if mode == "serial":
                    assert lib.ald_comm_gather_wait(comm, -1, C.byref(allw), C.byref(offs), C.byref(goffs)) == 0
                    t_land = time.perf_counter(); tm = []
                    for q in range(W):
                        t_ = time.perf_counter()
                        assert lib.ald_tset_add_stream(sink._h, C.cast(C.addressof(allw.contents) + 4 * offs[q], C.c_void_p), C.c_int64(offs[q + 1] - offs[q]), C.c_int32(goffs[q]), C.c_int64((k + 1) << 44)) == 0, lib.ald_last_error()
                        tm.append(time.perf_counter() - t_)
                    t_end = time.perf_counter()
                    rep.setdefault(mode, []).append((t_enq - t_begin, t_land - t_begin, sum(tm), t_end - t_begin, tm))
                else:
                    tm = []; tl = []
                    for q in range(W):                                   # stream q is merged as soon as it has landed, q + 1 .. still on their way
                        assert lib.ald_comm_gather_wait(comm, q, C.byref(allw), C.byref(offs), C.byref(goffs)) == 0
                        tl.append(time.perf_counter() - t_begin); t_ = time.perf_counter()
                        assert lib.ald_tset_add_stream(sink._h, C.cast(C.addressof(allw.contents) + 4 * offs[q], C.c_void_p), C.c_int64(offs[q + 1] - offs[q]), C.c_int32(goffs[q]), C.c_int64((k + 9) << 44)) == 0, lib.ald_last_error()
                        tm.append(time.perf_counter() - t_)
                    t_end = time.perf_counter()
                    rep.setdefault(mode, []).append((t_enq - t_begin, tl[-1], sum(tm), t_end - t_begin, tm))
        # the buffers exist twice: gather k + 1 is begun BEFORE gather k is merged -- a step then costs max(gather, merge), not their sum
        bar.wait(); t_all = time.perf_counter()
        assert lib.ald_comm_gather_begin(comm, C.c_void_p(src.data_ptr()), C.c_int64(src.numel()), C.c_int32(r * NG)) == 0, lib.ald_last_error()
        for k in range(STEPS):
            allw = C.POINTER(C.c_uint32)(); offs = C.POINTER(C.c_int64)(); goffs = C.POINTER(C.c_int32)()
            assert lib.ald_comm_gather_wait(comm, -1, C.byref(allw), C.byref(offs), C.byref(goffs)) == 0
            mine = [(C.addressof(allw.contents) + 4 * offs[q], offs[q + 1] - offs[q], goffs[q]) for q in range(W)] if r == 0 else []
            if k + 1 < STEPS:
                assert lib.ald_comm_gather_begin(comm, C.c_void_p(src.data_ptr()), C.c_int64(src.numel()), C.c_int32(r * NG)) == 0, lib.ald_last_error()
            for a, n, g0 in mine:
                assert lib.ald_tset_add_stream(sink._h, C.c_void_p(a), C.c_int64(n), C.c_int32(g0), C.c_int64((k + 17) << 44)) == 0, lib.ald_last_error()
        if r == 0: rep["double"] = (time.perf_counter() - t_all) / STEPS
        bar.wait()
        assert lib.ald_comm_destroy(comm) == 0
    except BaseException as e:
        err.append(e)
        try: bar.abort()
        except Exception: pass

ths = [threading.Thread(target=rank, args=(r,)) for r in range(W)]
for t in ths: t.start()
for t in ths: t.join()
if err: raise err[0]
tot_mb = sum(4 * s.numel() for s in streams) / 1e6
for mode in ("serial", "overlapped"):
    for k, (enq, land, merge, whole, tm) in enumerate(rep[mode]):
        print(f"{mode:10s} step {k}: begin returned after {1e3 * enq:7.1f} ms | all {W} streams ({tot_mb:.0f} MB) in pinned host memory after {1e3 * land:7.1f} ms | merge of the {W} streams {1e3 * merge:7.1f} ms ({', '.join('%.0f' % (1e3 * x) for x in tm)}) | step {1e3 * whole:7.1f} ms = {W * NG / whole / 1e6:.2f} M bundles/s through rank 0", flush=True)
print(f"double-buffered (gather k + 1 begun before gather k is merged): {1e3 * rep['double']:.1f} ms per step = {W * NG / rep['double'] / 1e6:.2f} M bundles/s through rank 0")
print(f"items in rank 0's set: {len(sink.items())}")
print("FUNNEL_OK")
