# the hub shapes (tests/shapes.py: single hubs of every fan size, k_in x k_out routers, hubs on chunk edges, graphs of twin size) GPU vs oracle,
# one library per child process:   python tools/hub_parity.py [lib.so ...]
# (tests/test_hub_shapes_gpu.py runs it on the STARREG=1, WSYNC=1 and ROWS=1 builds)
import sys
from parity_runner import run_libraries
CHILD = r'''
import shapes
tot = 0; nbad = 0
pg, _ = shapes.hub_batch(); wpg, _, wp = shapes.wide_router_batch(); zpg, _ = shapes.zero_count_batch()
for name, b, prm in (("hubs", pg, None), ("wide routers", wpg, wp), ("zero counts", zpg, None)):
    want = common.oracle_run(b, threads=threads, params=prm)[0]
    r = DR.run(b, prm); got = r.result
    bad = DR.oracle_mismatches(name, r, want)
    tot += b.n; nbad += len(bad)
    print("   batch", name, "graphs", b.n, "mismatch", bad[:3], "status", dict(zip(*[a.tolist() for a in np.unique(got.status, return_counts=True)])), flush=True)
print("   TOTAL graphs", tot, "mismatches", nbad, flush=True)
sys.exit(0 if nbad == 0 else 1)
'''
sys.exit(run_libraries(CHILD, sys.argv[1:]))
