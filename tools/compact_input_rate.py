# What compact input (ald_params.reserved & ALD_PARAM_COMPACT_INPUT / ALD_COMPACT_INPUT=1) does to the staging of a batch: wall ms of
# `add` (ald_batch_add_packed) and of `upload` (ald_batch_upload, which returns after the stream has drained, the expand kernels included),
# and the H2D bytes of the upload as the library's own log line states them (ALD_COMPACT_INPUT_LOG=1).
#
#   workload a   the bench batch: N x 64v/256e, seed 1002 as bench.py -- the caller supplies every column, only the in-CSR is derived
#   workload b   the same graphs handed over as assembler::assemble(bundle&) builds them: one sample per edge, the same one per graph,
#                abundance = weight, edge_abd / edge_count NULL -- the sample lists and both defaults are derived as well
#   modes        parent (the library of the parent commit, named by --parent-lib), head with the mode off, head with it on
#
# Every (mode, workload) runs in a process of its own (the mode is read when a batch is created and the library when it is loaded), ROUNDS
# times in alternation so that a drift of the machine shows in every mode alike; in a process: one discarded pass, then RUNS passes of
# clear / add / upload on ONE batch object, i.e. with warm pinned arrays, as a pipelined caller has them.
# Per line (mode, workload): min / max over all kept passes, and slowest-new over fastest-parent for the two head modes.
# Writes profiles/r14/compact_input_rate.json (--out) and prints the same JSON.
#
#   python tools/compact_input_rate.py --parent-lib <parent checkout>/aletsch_amd/lib/libaletsch_decomp.so
import argparse, dataclasses, json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 5


def uniform_of(pg, np):
    E = pg.g_ne.astype(np.int64)
    esoff = (np.arange(int(E.sum()) + pg.n, dtype=np.int64) - np.repeat(np.concatenate([[0], np.cumsum(E + 1)[:-1]]), E + 1)).astype(np.int32)
    return dataclasses.replace(pg, edge_sample_offset=esoff, sample_id=np.repeat(np.arange(pg.n, dtype=np.int32) % 3, E), sample_abd=pg.edge_weight.copy(), edge_count=None, edge_rank=None)


def child(workload, n):
    import numpy as np
    import aletsch_amd as A
    pg = A.synth(seed=1002, n_graphs=n, v_min=64, v_max=64, fixed_edges=256)
    args = list(pg.c_args())
    if workload == "b":
        pg = uniform_of(pg, np); args = list(pg.c_args()); args[8] = None          # edge_abd NULL (edge_count already is)
    lib = A.load_library(); runs = []
    with A.DecompBatch(0) as b:
        for i in range(RUNS + 1):
            t0 = time.perf_counter()
            b.clear()
            t1 = time.perf_counter()
            rc = lib.ald_batch_add_packed(b._h, *args); assert rc == 0, rc
            t2 = time.perf_counter()
            b.upload()
            t3 = time.perf_counter()
            runs.append(dict(clear_ms=round(1e3 * (t1 - t0), 3), add_ms=round(1e3 * (t2 - t1), 3), upload_ms=round(1e3 * (t3 - t2), 3)))
        b.run(); b.download(); paths = int(b.result().path_offset[-1])                # the staged batch is a batch the kernels take
        alg = b.algorithmic_bytes()[0]
    print(json.dumps(dict(runs=runs[1:], paths=paths, algorithmic_in_bytes=alg, n_graphs=n)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None); ap.add_argument("--graphs", type=int, default=100000); ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default=os.environ.get("PARENT_LIB")); ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "compact_input_rate.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.graphs)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("compact_input_rate: --parent-lib must name the parent commit's libaletsch_decomp.so")
    modes = (("parent", dict(ALETSCH_DECOMP_LIB=a.parent_lib)), ("head_off", dict(ALD_COMPACT_INPUT="0")), ("head_on", dict(ALD_COMPACT_INPUT="1", ALD_COMPACT_INPUT_LOG="1")))
    res = dict(tool="compact_input_rate", n_graphs=a.graphs, runs_per_process=RUNS, rounds=a.rounds, lines={})
    for rnd in range(a.rounds):
        for wl in ("a", "b"):
            for mode, env in modes:
                e = {k: v for k, v in os.environ.items() if k not in ("ALETSCH_DECOMP_LIB", "ALD_COMPACT_INPUT", "ALD_COMPACT_INPUT_LOG")}; e.update(env)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", wl, "--graphs", str(a.graphs)], capture_output=True, text=True, env=e, timeout=600)
                if r.returncode != 0:
                    sys.exit("compact_input_rate: %s / %s failed:\n%s" % (mode, wl, r.stderr[-3000:]))
                out = json.loads(r.stdout.strip().splitlines()[-1])
                line = res["lines"].setdefault(mode + "/" + wl, dict(runs=[], paths=out["paths"], algorithmic_in_bytes=out["algorithmic_in_bytes"]))
                assert line["paths"] == out["paths"]
                line["runs"] += out["runs"]
                logs = [re.search(r"elided((?: [A-Z]+)*) sent (\d+) full (\d+) expand_ms ([0-9.]+)", ln) for ln in r.stderr.splitlines() if "compact upload" in ln]
                if logs:
                    m = logs[-1]
                    line.update(elided=m.group(1).split(), h2d_bytes=int(m.group(2)), h2d_bytes_full=int(m.group(3)))
                    line.setdefault("expand_ms", []).extend(float(x.group(4)) for x in logs[1:])      # (the first upload of a process is the discarded pass)
    for key, line in res["lines"].items():
        for f in ("add_ms", "upload_ms"):
            v = [x[f] for x in line["runs"]]; line[f + "_min_max"] = [min(v), max(v)]
        v = [x["add_ms"] + x["upload_ms"] for x in line["runs"]]; line["add_plus_upload_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
        if "h2d_bytes" in line:
            line["h2d_bytes_per_graph"] = round(line["h2d_bytes"] / a.graphs, 1); line["h2d_bytes_full_per_graph"] = round(line["h2d_bytes_full"] / a.graphs, 1)
    for wl in ("a", "b"):
        assert len({res["lines"][m + "/" + wl]["paths"] for m, _ in modes}) == 1, "the modes disagree on the number of paths"
        par = res["lines"]["parent/" + wl]
        for mode in ("head_off", "head_on"):
            new = res["lines"][mode + "/" + wl]
            new["slowest_new_over_fastest_parent"] = {f: round(new[f + "_min_max"][1] / par[f + "_min_max"][0], 3) for f in ("add_ms", "upload_ms", "add_plus_upload_ms")}
        par["own_spread_slowest_over_fastest"] = {f: round(par[f + "_min_max"][1] / par[f + "_min_max"][0], 3) for f in ("add_ms", "upload_ms", "add_plus_upload_ms")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
