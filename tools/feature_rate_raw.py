# The transcript feature block of a batch of RAW graphs (as assembler::assemble(gx, px, sid) receives them): ald_batch_features_all_ex with
# ALD_FEAT_RAW_ON_DEVICE (the wave of a raw graph folds its boundaries into an overlay and computes the rows: trst_features_dev.h) against the
# same call without the flag (the host routine ald_batch_features for every raw graph -- pre-steps, re-staging, rows -- on up to 16 host
# threads inside the call), on the SAME downloaded batch in the same process:
#   N (environment, default 20 000) graphs of tests/common.py's gene_like_raw (3..9 exon runs), max_group_boundary_distance from
#   [10000, 10000, 150, 0], random extras.  Graphs on which the pre-steps assert are left out of the draw: they have no rows either way, and
#   only the host routine reports the assert a second time in graph_rc.
# One untimed first call each (it allocates), then three timed calls each; call_ms is the library's own wall clock of the whole call,
# device_kernel_ms the kernel's events.  The two tables must agree bit for bit (rows, complete, graph_rc, row_begin).
# Writes one JSON line to profiles/r07/feature_rate_raw.json (and stdout); exit status 1 on disagreement.
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aletsch_amd as A
from aletsch_amd.packed import PackedGraphs
import common


def draw(n, seed=7):
    rng = np.random.default_rng(seed)
    items = []; t = 0; asserted = 0
    while len(items) < n:
        g, phases = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 10)), strand="+-."[t % 3]); t += 1
        pg = PackedGraphs.from_graphs([g])
        pg.edge_rank = np.array(sorted(range(len(g["edges"])), key=lambda k: (g["edges"][k][0], g["edges"][k][1])), np.int32)
        pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
        dist = int(rng.choice([10000, 10000, 150, 0]))
        if A.pre_assemble(pg, phases, dist)[3]:
            asserted += 1; continue
        items.append((pg, phases, dist))
    return items, asserted


def timed(b, bx, g_nv, flag, reps=3):
    call, kern, host = [], [], []
    for _ in range(reps + 1):                                       # the first call allocates the table and its buffers
        t = b.features_all(bx, raw_on_device=flag)
        call.append(t["stats"]["call_ms"]); kern.append(t["stats"]["device_ms"]); host.append(int(t["stats"]["host_graphs"]))
    return t, {"call_ms": [round(x, 3) for x in call[1:]], "first_call_ms": round(call[0], 3), "device_kernel_ms": [round(x, 3) for x in kern[1:]], "host_graphs": host[-1]}


def main():
    n = int(os.environ.get("N", "20000"))
    items, asserted = draw(n)
    rng = np.random.default_rng(11)
    with A.DecompBatch(0) as b:
        for pg, phases, dist in items:
            assert b.add_raw(pg, phases, dist) == 0
        b.upload(); b.run(); b.download()
        g_nv = np.array([int(it[0].g_nv[0]) for it in items]); TV = int(g_nv.sum())
        bx = A.BatchExtras.from_arrays(boundary_loss1=rng.random(TV), boundary_loss2=rng.random(TV), boundary_loss3=rng.random(TV), boundary_merged_loss=rng.random(TV),
                                       unbridge_leaving_count=rng.integers(0, 9, TV), unbridge_leaving_ratio=rng.random(TV),
                                       unbridge_coming_count=rng.integers(0, 9, TV), unbridge_coming_ratio=rng.random(TV),
                                       gr_reads=rng.integers(1, 10000, n), gr_subgraph=rng.integers(0, 4, n))
        t_off, off = timed(b, bx, g_nv, False)
        t_on, on = timed(b, bx, g_nv, True)
    # field by field (the padding of a row is nobody's); where the reference would have asserted in the features the partial row means nothing
    skip = np.zeros(len(t_off["complete"]), bool)
    for g in np.nonzero(t_off["graph_rc"] != 0)[0]:
        skip[t_off["row_begin"][g]:t_off["row_begin"][g + 1]] = True
    differ = [k for k in ("row_begin", "graph_rc", "complete") if not np.array_equal(t_off[k], t_on[k])]
    if "row_begin" not in differ:
        differ += [f for f in A.FEATURE_DTYPE.names if not np.array_equal(t_off["rows"][f][~skip].view(np.uint8), t_on["rows"][f][~skip].view(np.uint8))]
    agree = not differ
    out = {"tool": "feature_rate_raw", "graphs": n, "left_out_asserting": asserted, "vertices": int(g_nv.sum()), "edges": int(sum(int(it[0].g_ne[0]) for it in items)),
           "rows": int(t_on["row_begin"][-1]), "agree_bit_for_bit": agree, "fields_that_differ": differ, "asserted_graphs": int((t_off["graph_rc"] != 0).sum()), "flag_off": off, "flag_on": on,
           "slowest_on_over_fastest_off": round(max(on["call_ms"]) / min(off["call_ms"]), 4), "accepted": bool(agree and max(on["call_ms"]) < min(off["call_ms"])),
           "note": "call_ms = wall clock of the whole call inside the library (path table, extras upload, kernel, the table's D2H; flag off: plus the host routine on up to 16 threads); "
                   "flag_off is the code path of ald_batch_features_all, unchanged"}
    line = json.dumps(out)
    print(line)
    d = os.path.join(ROOT, "profiles", "r07"); os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "feature_rate_raw.json"), "w") as f:
        f.write(line + "\n")
    return 0 if agree else 1


if __name__ == "__main__":
    sys.exit(main())
