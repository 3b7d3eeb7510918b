# the slab-resident twins (classes 11 / 12) on their own, GPU vs oracle: graphs of 385..512 vertices with ALD_DEBUG_TWIN=1 (every graph of
# classes 7 / 8 goes to its twin), one library per child process:   python tools/twins_parity.py [lib.so ...]
# (tests/test_gpu_parity.py::test_register_form_of_the_small_fans_on_the_twins runs it on the STARREG=1 build and on the product)
import sys
from parity_runner import run_libraries
CHILD = r'''
tot = 0; nbad = 0; ntwin = 0
for seed, epv in ((11, 3), (12, 3), (13, 4), (14, 2)):
    pg = A.synth(seed=seed, n_graphs=50, v_min=385, v_max=512, edges_per_vertex=epv)
    want = common.oracle_run(pg, threads=threads)[0]
    r = DR.run(pg); got = r.result; info = r.classes
    bad = DR.oracle_mismatches("seed %d" % seed, r, want)
    tot += pg.n; nbad += len(bad); ntwin += info.get(11, 0) + info.get(12, 0)
    print("   seed", seed, "classes", info, "mismatch", len(bad), "status", dict(zip(*[a.tolist() for a in np.unique(got.status, return_counts=True)])), flush=True)
print("   TOTAL graphs", tot, "on the twins", ntwin, "mismatches", nbad, flush=True)
sys.exit(0 if nbad == 0 and ntwin == tot else 1)
'''
sys.exit(run_libraries(CHILD, sys.argv[1:], env={"ALD_DEBUG_TWIN": "1"}))
