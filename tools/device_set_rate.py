# The end-to-end rate of bench.py's sink_pipeline (stage | kernel | download | merge into ONE persistent set, four host threads,
# 6 x 100 000 x 64v/256e, skip_single_exon on) for four merge paths in one process:
#   host_sink      ald_tset_add_batch into the host sink (the product path)
#   gpu_reduction  ald_batch_reduce_transcripts + ald_tset_add_flat (row f3)
#   device_set     ald_tset_dev_add_batch into a set resident in HBM; one snapshot at the end is timed in
#   device_set_finish   the same loop with ald_batch_finish in the place of ald_batch_download: no record comes to the host
# Prints one JSON line: bundles/s and ms per batch per mode, for the device sets the device / wall milliseconds of every add, the bytes the
# run-ending call moved to the host per batch, its mean stage times (ALD_DOWNLOAD_PROF-style, host milliseconds) and the milliseconds per
# batch every pipeline thread spent working (stage = clear + add + upload, kernel = run + sync, end = download / finish, merge).
import json, os, queue, sys, threading, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aletsch_amd as A

N = int(os.environ.get("N", "100000")); ROUNDS = int(os.environ.get("ROUNDS", "6"))


def run(mode, pg, n, rounds):
    sid = (np.arange(n) % 8).astype(np.int32)
    batches = [A.DecompBatch(0) for _ in range(4)]
    for b in batches:
        b.add(pg); b.upload(); b.run(); b.download(); b.clear()
    free = queue.Queue(); staged = queue.Queue(maxsize=1); ran = queue.Queue(maxsize=1); done = queue.Queue(maxsize=1)
    for b in batches:
        free.put(b)
    on_device = mode in ("device_set", "device_set_finish")
    sink = A.TranscriptSink(0.8); ds = A.DeviceTranscriptSet(0, 0.8) if on_device else None
    err = []; adds = []; ends = []
    busy = {"stage": 0.0, "kernel": 0.0, "end": 0.0, "merge": 0.0}      # seconds every stage's thread spent working (not waiting for a batch)

    def timed(name, f):
        def g(b):
            t = time.perf_counter(); f(b); busy[name] += time.perf_counter() - t
        return g

    def relay(src, dst, step):                              # one pipeline stage on its own thread; None ends the stream
        try:
            while True:
                b = src.get()
                if b is None:
                    break
                step(b); dst.put(b)
        except BaseException as e:
            err.append(e)
        dst.put(None)

    def stage():
        try:
            for _ in range(rounds):
                b = free.get(); timed("stage", lambda x: (x.clear(), x.add(pg), x.upload()))(b); staged.put(b)
        except BaseException as e:
            err.append(e)
        staged.put(None)

    kern = lambda: relay(staged, ran, timed("kernel", lambda b: (b.run(), b.sync())))        # the kernel of batch k + 1 runs while batch k is copied back
    def end(b):                                             # the call that ends the run, and what it moved to the host
        if mode == "device_set_finish":
            b.finish(); ends.append(b.last_finish_ms())
        else:
            b.download(); ends.append(b.download_ms())
    fetch = lambda: relay(ran, done, timed("end", end))

    def merge():
        r = 0
        try:
            while True:
                b = done.get()
                if b is None:
                    break
                t = time.perf_counter()
                if on_device:
                    ds.add_batch(b, sid, tid_base=r << 44, skip_single_exon=True); adds.append(ds.stats())
                elif mode == "gpu_reduction":
                    b.reduce_into(sink, sid, tid_base=r << 44, skip_single_exon=True)
                else:
                    sink.add_batch(b, sid, tid_base=r << 44, skip_single_exon=True)
                busy["merge"] += time.perf_counter() - t
                r += 1; free.put(b)
            if on_device:                                      # the result leaves the device once, at the end
                t = time.perf_counter(); ds.snapshot_into(sink); adds.append({"snapshot_ms": 1e3 * (time.perf_counter() - t)})
        except BaseException as e:
            err.append(e)
            while done.get() is not None:
                pass
    ths = [threading.Thread(target=f, daemon=True) for f in (stage, kern, fetch, merge)]
    t0 = time.perf_counter()
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    el = time.perf_counter() - t0
    if err:
        raise err[0]
    out = {"bundles_per_s": rounds * n / el, "ms_per_batch": 1e3 * el / rounds, "bytes_to_host_per_batch": int(np.mean([e["bytes_to_host"] for e in ends])),
           "end_of_run_ms": {k: round(float(np.mean([e[k] for e in ends])), 2) for k in ends[0] if k != "bytes_to_host"},
           "busy_ms_per_batch": {k: round(1e3 * v / rounds, 2) for k, v in busy.items()}}      # the stage with the largest figure bounds the loop
    if ds is not None:
        out["device_ms_per_add"] = [round(a["device_ms"], 2) for a in adds if "device_ms" in a]
        out["call_ms_per_add"] = [round(a["call_ms"], 2) for a in adds if "call_ms" in a]
        out["snapshot_ms"] = round(adds[-1]["snapshot_ms"], 2)
        out["device_items"] = adds[-2]["device_items"] if len(adds) > 1 else None
        ds.close()
    sink.close()
    for b in batches:
        b.close()
    return out


def main():
    pg = A.synth(seed=1002, n_graphs=N, v_min=64, v_max=64, fixed_edges=256)
    res = {"workload": f"{ROUNDS} batches of {N} graphs (64v/256e) through stage | kernel | download | merge into one persistent transcript set, "
                       "skip_single_exon on, four host threads (bench.py sink_pipeline); device_set_finish ends the run with ald_batch_finish instead"}
    for mode in ("host_sink", "gpu_reduction", "device_set", "device_set_finish"):
        res[mode] = run(mode, pg, N, ROUNDS)
        print(mode, json.dumps(res[mode]), file=sys.stderr, flush=True)
    res["device_set_over_host_sink"] = res["device_set"]["bundles_per_s"] / res["host_sink"]["bundles_per_s"]
    res["device_set_finish_over_device_set"] = res["device_set_finish"]["bundles_per_s"] / res["device_set"]["bundles_per_s"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
