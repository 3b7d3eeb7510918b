# The end-to-end rate of bench.py's sink_pipeline (stage | kernel | download | merge into ONE persistent set, four host threads,
# 6 x 100 000 x 64v/256e, skip_single_exon on) for three merge paths in one process:
#   host_sink      ald_tset_add_batch into the host sink (the product path)
#   gpu_reduction  ald_batch_reduce_transcripts + ald_tset_add_flat (row f3)
#   device_set     ald_tset_dev_add_batch into a set resident in HBM; one snapshot at the end is timed in
# Prints one JSON line: bundles/s and ms per batch per mode, and for device_set the device / wall milliseconds of every add.
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
    sink = A.TranscriptSink(0.8); ds = A.DeviceTranscriptSet(0, 0.8) if mode == "device_set" else None
    err = []; adds = []

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
                b = free.get(); b.clear(); b.add(pg); b.upload(); staged.put(b)
        except BaseException as e:
            err.append(e)
        staged.put(None)

    kern = lambda: relay(staged, ran, lambda b: (b.run(), b.sync()))        # the kernel of batch k + 1 runs while batch k is copied back
    fetch = lambda: relay(ran, done, lambda b: b.download())

    def merge():
        r = 0
        try:
            while True:
                b = done.get()
                if b is None:
                    break
                if mode == "device_set":
                    ds.add_batch(b, sid, tid_base=r << 44, skip_single_exon=True); adds.append(ds.stats())
                elif mode == "gpu_reduction":
                    b.reduce_into(sink, sid, tid_base=r << 44, skip_single_exon=True)
                else:
                    sink.add_batch(b, sid, tid_base=r << 44, skip_single_exon=True)
                r += 1; free.put(b)
            if mode == "device_set":                           # the result leaves the device once, at the end
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
    out = {"bundles_per_s": rounds * n / el, "ms_per_batch": 1e3 * el / rounds}
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
                       "skip_single_exon on, four host threads (bench.py sink_pipeline)"}
    for mode in ("host_sink", "gpu_reduction", "device_set"):
        res[mode] = run(mode, pg, N, ROUNDS)
        print(mode, json.dumps(res[mode]), file=sys.stderr, flush=True)
    res["device_set_over_host_sink"] = res["device_set"]["bundles_per_s"] / res["host_sink"]["bundles_per_s"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
