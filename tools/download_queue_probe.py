# Does a download wait for ANOTHER batch's kernel?  Four resident batch objects at the bench shape rotate as bench.py's main thread
# drives them -- prev.sync(); cur.run(); prev.download() -- and every download is kept apart PER BATCH OBJECT: which hardware queue a
# stream lands on is fixed when the stream is created, so a collision between one batch's result copies and the queue a neighbour's class
# kernel runs on shows as ONE object of the four whose `status_retries` part is a whole kernel long, step after step, while the mean over
# all downloads (what bench.py reports) only shows a quarter of it.
#
# Per batch object: min / median / max of the four parts of ald_batch_last_download_ms (wait for the kernel, status + retries, D2H
# copies, decode), of the kernel's own time (HIP events) and of the kernel PERIOD: host time between the moments two successive kernels
# were seen finished (prev.sync() returning), booked to the batch whose kernel ended the interval.  Period - kernel = GPU idle per step.
# The first rotation is discarded.  The environment is taken as it is (GPU_MAX_HW_QUEUES, ALD_DOWNLOAD_STREAM, ALETSCH_DECOMP_LIB): run
# it once per arrangement and name the arrangement with --label.  Prints a table, then one JSON line.
#
#   python tools/download_queue_probe.py --label head                                   >> profiles/rNN/download_queue_probe.txt
#   ALETSCH_DECOMP_LIB=<parent checkout>/aletsch_amd/lib/libaletsch_decomp.so python tools/download_queue_probe.py --label parent
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("wait_kernel", "status_retries", "copy", "decode")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="head"); ap.add_argument("--graphs", type=int, default=100000); ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rotations", type=int, default=6, help="timed rotations over the batch objects (one more, the first, is discarded)")
    a = ap.parse_args()
    import aletsch_amd as A
    pg = A.synth(seed=1002, n_graphs=a.graphs, v_min=64, v_max=64, fixed_edges=256)          # bench.py's batch
    batches = [A.DecompBatch(0) for _ in range(a.batches)]
    for b in batches:
        b.add(pg); b.upload(); b.run(); b.download()
    paths = int(batches[0].result().path_offset[-1])
    rows = [dict((k, []) for k in PARTS + ("kernel", "period")) for _ in batches]
    prev = None; seen = None
    for step in range((a.rotations + 1) * a.batches + 1):
        i = step % a.batches; cur = batches[i]; keep = step > a.batches
        if prev is not None:
            batches[prev].sync()
            now = time.perf_counter()
            if keep and seen is not None:
                rows[prev]["period"].append(1e3 * (now - seen))
            seen = now
        cur.run()
        if prev is not None:
            batches[prev].download()
            if keep:
                d = batches[prev].download_ms()
                for k in PARTS:
                    rows[prev][k].append(d[k])
                rows[prev]["kernel"].append(batches[prev].kernel_ms())
        prev = i
    batches[prev].download()
    assert all(int(b.result().path_offset[-1]) == paths for b in batches), "the batch objects disagree on the number of paths"
    for b in batches:
        b.close()
    env = {k: os.environ.get(k) for k in ("GPU_MAX_HW_QUEUES", "ALD_DOWNLOAD_STREAM", "ALD_UPLOAD_STREAM")}
    env["ALETSCH_DECOMP_LIB"] = "set" if os.environ.get("ALETSCH_DECOMP_LIB") else None      # (another library than the tree's: the label says which)
    out = dict(tool="download_queue_probe", label=a.label, env=env, n_graphs=a.graphs, paths=paths, samples_per_batch=a.rotations, batches=[])
    print("# %s: %d batch objects x %d graphs (64v/256e), %d downloads each; ms as min / median / max; env %s" % (a.label, a.batches, a.graphs, a.rotations, json.dumps(env)))
    print("# %-6s %-8s" % (a.label, "batch") + "".join(" %-24s" % k for k in PARTS + ("kernel", "period")))
    for i, r in enumerate(rows):
        s = {k: [round(min(v), 3), round(statistics.median(v), 3), round(max(v), 3)] for k, v in r.items()}
        out["batches"].append(s)
        print("  %-6s %-8d" % (a.label, i) + "".join(" %-24s" % ("%.2f / %.2f / %.2f" % tuple(s[k])) for k in PARTS + ("kernel", "period")))
    allp = [x for r in rows for x in r["period"]]; allk = [x for r in rows for x in r["kernel"]]
    out["period_ms_mean"] = round(statistics.mean(allp), 3); out["kernel_ms_mean"] = round(statistics.mean(allk), 3)      # (one slow object in four does not move a median)
    out["status_retries_ms_max"] = round(max(x for r in rows for x in r["status_retries"]), 3)
    print("# %-6s kernel period mean %.2f ms, kernel mean %.2f ms, largest status part %.2f ms" % (a.label, out["period_ms_mean"], out["kernel_ms_mean"], out["status_retries_ms_max"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
