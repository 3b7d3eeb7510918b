# The transcript feature block of a whole batch: ald_batch_features_all (one device pass, trst_features.hip) against the per-graph host
# routine ald_batch_features called for every graph in turn on ONE thread, on
#   real_shaped  100 000 graphs of ~64 vertices with touching exon runs (synth layout_mode=1, as test_transcript_features_match_oracle)
#   cfg3_mixed   10 000 graphs, V ~ U{8..512}, E = 4V (BASELINE.json configs[2]), layout_mode=1
# with random extras.  The device call is timed by its own events (kernel) and by the wall clock (the whole call: path table, extras
# upload, kernel, the table's copy back); the host loop by the wall clock, minus nothing -- the ctypes cost of the calls is measured
# separately (the same loop over ald_batch_get_result) and reported, not subtracted.  The two tables must agree bit for bit.
# One thread for the host loop: concurrent calls on one batch are safe (ald_batch_features only reads it), but the reference calls
# update_trst_features inside its single-threaded per-bundle assemble, so one thread is the host routine's fair unit.
# Writes one JSON line to profiles/r06/feature_rate.json (and stdout).
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aletsch_amd as A
from aletsch_amd.native import _ResultView


def extras_for(pg, rng):
    TV = int(pg.g_nv.sum())
    return A.BatchExtras.from_arrays(boundary_loss1=rng.random(TV), boundary_loss2=rng.random(TV), boundary_loss3=rng.random(TV), boundary_merged_loss=rng.random(TV),
                                     unbridge_leaving_count=rng.integers(0, 9, TV), unbridge_leaving_ratio=rng.random(TV),
                                     unbridge_coming_count=rng.integers(0, 9, TV), unbridge_coming_ratio=rng.random(TV),
                                     gr_reads=rng.integers(1, 10000, pg.n), gr_subgraph=rng.integers(0, 4, pg.n))


def host_loop(b, n, bx, total, g_nv):
    """ald_batch_features for every graph, one thread, straight into one table"""
    lib = b._lib
    rows = np.zeros(max(total, 1), A.FEATURE_DTYPE); comp = np.zeros(max(total, 1), np.int32); rc = np.zeros(n, np.int32)
    off = np.concatenate([[0], np.cumsum(np.asarray(g_nv, np.int64))]).astype(np.int64)
    gx = A.GraphExtras(); rb = np.zeros(n + 1, np.int64); rv = _ResultView()
    names = [k for k in A.BatchExtras.VERTEX_FIELDS if k in bx.arrays]
    base_r, base_c = rows.ctypes.data, comp.ctypes.data
    t0 = time.perf_counter()
    for g in range(n):
        lib.ald_batch_get_result(b._h, g, C.byref(rv))
        for k in names:
            a = bx.arrays[k]
            setattr(gx, k, C.cast(a.ctypes.data + a.itemsize * int(off[g]), type(getattr(gx, k))))
        gx.gr_reads = int(bx.arrays["gr_reads"][g]); gx.gr_subgraph = int(bx.arrays["gr_subgraph"][g])
        r0 = int(rb[g]); rb[g + 1] = r0 + rv.num_paths
        rc[g] = lib.ald_batch_features(b._h, g, C.byref(gx), C.c_void_p(base_r + A.FEATURE_DTYPE.itemsize * r0), C.c_void_p(base_c + 4 * r0))
    host_s = time.perf_counter() - t0
    # the same loop without the feature routine: what the Python / ctypes side of it costs
    t0 = time.perf_counter()
    for g in range(n):
        lib.ald_batch_get_result(b._h, g, C.byref(rv))
        for k in names:
            a = bx.arrays[k]
            setattr(gx, k, C.cast(a.ctypes.data + a.itemsize * int(off[g]), type(getattr(gx, k))))
        gx.gr_reads = int(bx.arrays["gr_reads"][g]); gx.gr_subgraph = int(bx.arrays["gr_subgraph"][g])
        lib.ald_batch_get_result(b._h, g, C.byref(rv))
    loop_s = time.perf_counter() - t0
    return rows[:total], comp[:total], rc, rb, host_s, loop_s


def measure(name, pg, reps=3):
    rng = np.random.default_rng(7)
    bx = extras_for(pg, rng)
    with A.DecompBatch(0) as b:
        b.add(pg); b.upload(); b.run(); b.download()
        walls, devs, insides = [], [], []
        for _ in range(reps + 1):                                   # the first call allocates the table and its buffers
            t0 = time.perf_counter()
            rc_call = b._lib.ald_batch_features_all(b._h, C.byref(bx))
            walls.append(1e3 * (time.perf_counter() - t0))
            assert rc_call == 0, rc_call
            st = [C.c_double(), C.c_double(), C.c_int64(), C.c_int64()]
            b._lib.ald_batch_features_stats(b._h, *[C.byref(x) for x in st])
            devs.append(st[0].value); insides.append(st[1].value)
        t0 = time.perf_counter()
        got = b.features_table()                                    # the Python view: a numpy copy of the whole table
        copy_ms = 1e3 * (time.perf_counter() - t0)
        total = int(got["row_begin"][-1])
        rows, comp, rc, rb, host_s, loop_s = host_loop(b, pg.n, bx, total, pg.g_nv)
    skip = np.zeros(total, bool)
    for g in np.nonzero(rc != 0)[0]:
        skip[rb[g]:rb[g + 1]] = True
    agree = bool(np.array_equal(rb, got["row_begin"]) and np.array_equal(rc, got["graph_rc"]) and np.array_equal(comp, got["complete"])
                 and all(np.array_equal(rows[f][~skip].view(np.uint8), got["rows"][f][~skip].view(np.uint8)) for f in A.FEATURE_DTYPE.names))
    return {"graphs": pg.n, "rows": total, "asserted_graphs": int((rc != 0).sum()), "agree_bit_for_bit": agree,
            "device_kernel_ms": [round(x, 3) for x in devs[1:]], "device_call_ms": [round(x, 3) for x in walls[1:]], "device_first_call_ms": round(walls[0], 3),
            "call_ms_inside_library": [round(x, 3) for x in insides[1:]], "python_table_copy_ms": round(copy_ms, 1),
            "host_loop_ms_one_thread": round(1e3 * host_s, 1), "host_loop_ctypes_overhead_ms": round(1e3 * loop_s, 1),
            "speedup_call_vs_host_loop": round(1e3 * host_s / min(walls[1:]), 1)}


def main():
    out = {"tool": "feature_rate", "note": "device = ald_batch_features_all through ctypes (kernel events; the whole call by wall clock: path table, "
                                           "extras upload, kernel, the table's D2H into pinned memory); python_table_copy_ms = DecompBatch.features_table's numpy copy, "
                                           "not part of the call; host = ald_batch_features per graph on one thread (wall clock, ctypes cost of the loop reported separately)"}
    n = int(os.environ.get("N", "100000"))
    out["real_shaped"] = measure("real_shaped", A.synth(seed=52, n_graphs=n, v_min=56, v_max=72, edges_per_vertex=3, layout_mode=1, weight_mode=2,
                                                        phasing_per_graph=3, n_samples=3))
    out["cfg3_mixed"] = measure("cfg3_mixed", A.synth(seed=1003, n_graphs=max(n // 10, 1), v_min=8, v_max=512, edges_per_vertex=4, layout_mode=1))
    line = json.dumps(out)
    print(line)
    d = os.path.join(ROOT, "profiles", "r06"); os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "feature_rate.json"), "w") as f:
        f.write(line + "\n")
    return 0 if out["real_shaped"]["agree_bit_for_bit"] and out["cfg3_mixed"]["agree_bit_for_bit"] else 1


if __name__ == "__main__":
    sys.exit(main())
