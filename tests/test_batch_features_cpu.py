"""CPU tier of the batched feature pass (ald_batch_features_all): the per-graph routine of the kernel (aletsch_amd/csrc/trst_features_dev.h),
compiled with g++ under -DALD_EMU (tests/feature_emu), fed the oracle's paths, against the oracle's restatement of
scallop::update_trst_features + unique_junc: every field of every complete row bit for bit, the complete flags, the asserted graphs; with
the junction lists in LDS and in the scratch.  And the ABI surface of the new entry points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aletsch_amd as A
import common
from aletsch_amd.packed import PackedGraphs

_FEMU = None


def femu_lib():
    global _FEMU
    if _FEMU is None:
        path = os.path.join(common.ROOT, "tests", "_build", "libfeature_emu.so")
        src = [os.path.join(common.ROOT, "aletsch_amd", "csrc", f) for f in ("trst_features_dev.h", "decomp_common.h", "host_pack.h")] + [os.path.join(common.ROOT, "tests", "feature_emu", "feature_emu.cc")]
        if not os.path.exists(path) or any(os.path.getmtime(f) > os.path.getmtime(path) for f in src):
            subprocess.run(["make", "-C", os.path.join(common.ROOT, "tests", "feature_emu")], check=True, stdout=subprocess.DEVNULL)
        _FEMU = C.CDLL(path)
    return _FEMU


def emu_features(pg: PackedGraphs, res, extras=None, lds_words=4096):
    """the device routine on one lane over the oracle's paths -> (rows, complete, graph_rc)"""
    L = femu_lib()
    path_offset = np.asarray(res.path_offset, np.int64); pv_offset = np.asarray(res.pv_offset, np.int64)
    pv = np.ascontiguousarray(res.path_vertices, np.int32)
    m = int(path_offset[-1])
    rows = np.zeros(max(m, 1), A.FEATURE_DTYPE); comp = np.zeros(max(m, 1), np.int32); rc = np.zeros(pg.n, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    rc_call = L.femu_features(*pg.c_args(), p(path_offset), p(pv_offset), p(pv), C.byref(extras) if extras is not None else None, C.c_int32(lds_words),
                              p(rows), p(comp), p(rc))
    assert rc_call == 0
    return rows[:m], comp[:m], rc


def random_extras(pg, rng):
    TV = int(pg.g_nv.sum())
    return A.BatchExtras.from_arrays(boundary_loss1=rng.random(TV), boundary_loss2=rng.random(TV), boundary_loss3=rng.random(TV), boundary_merged_loss=rng.random(TV),
                                     unbridge_leaving_count=rng.integers(0, 9, TV), unbridge_leaving_ratio=rng.random(TV),
                                     unbridge_coming_count=rng.integers(0, 9, TV), unbridge_coming_ratio=rng.random(TV),
                                     gr_reads=rng.integers(1, 10000, pg.n), gr_subgraph=rng.integers(0, 4, pg.n))


def per_graph_extras(pg, bx):
    off = np.concatenate([[0], np.cumsum(pg.g_nv)])
    out = []
    for g in range(pg.n):
        kw = {k: v[off[g]:off[g + 1]] for k, v in bx.arrays.items() if k not in ("gr_reads", "gr_subgraph")}
        out.append(A.GraphExtras.from_arrays(gr_reads=int(bx.arrays["gr_reads"][g]), gr_subgraph=int(bx.arrays["gr_subgraph"][g]), **kw))
    return out


def check_against_oracle(pg, extras=None):
    res, want = common.oracle_features(pg, per_graph_extras(pg, extras) if extras is not None else None)
    stats = dict(complete=0, single=0, asserted=0, intron=0)
    tables = [emu_features(pg, res, extras, lds) for lds in (4096, 0)]       # junction lists in LDS / all in the scratch
    for rows, comp, rc in tables:
        for g in range(pg.n):
            wf, wc, wbad = want[g]
            assert (rc[g] != 0) == wbad, (g, rc[g], wbad)
            r0, r1 = int(res.path_offset[g]), int(res.path_offset[g + 1])
            assert r1 - r0 == len(wc)
            if wbad:
                stats["asserted"] += 1; continue
            assert np.array_equal(comp[r0:r1], wc), g
            for k in range(len(wc)):
                d = {x: rows[r0 + k][x].item() for x in A.FEATURE_DTYPE.names}
                if wc[k]:
                    bad = {x: (d[x], wf[k][x]) for x in d if np.float64(d[x]).tobytes() != np.float64(wf[k][x]).tobytes() and d[x] != wf[k][x]}
                    assert d == wf[k], (g, k, bad)
                    stats["complete"] += 1; stats["intron"] += int(d["introns"] + d["start_introns"] + d["end_introns"] > 0)
                else:
                    for x in ("gr_vertices", "gr_edges", "gr_reads", "gr_subgraph", "num_vertices", "num_edges", "max_mid_exon_len"):
                        assert d[x] == wf[k][x]
                    stats["single"] += 1
    for name in A.FEATURE_DTYPE.names:                                     # both placements give the same bits
        a, b = tables[0][0][name], tables[1][0][name]
        assert a.tobytes() == b.tobytes(), name
    assert np.array_equal(tables[0][2], tables[1][2])
    return stats


def test_device_routine_matches_oracle_multi_sample():
    pg = A.synth(seed=52, n_graphs=300, v_min=8, v_max=70, edges_per_vertex=3, layout_mode=1, weight_mode=2, phasing_per_graph=3, n_samples=3)
    rng = np.random.default_rng(3)
    pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
    s = check_against_oracle(pg, random_extras(pg, rng))
    assert s["complete"] > 1000 and s["single"] > 0 and s["intron"] > 0, s


def test_device_routine_matches_oracle_without_extras():
    pg = A.synth(seed=57, n_graphs=200, v_min=6, v_max=120, edges_per_vertex=4, layout_mode=1, weight_mode=1, n_samples=5)
    rng = np.random.default_rng(8)
    pg.edge_count = (pg.sample_counts() + rng.integers(0, 5, pg.edge_target.size)).astype(np.int32)
    s = check_against_oracle(pg, None)
    assert s["complete"] > 500, s


def test_device_routine_with_parallel_edges():
    rng = np.random.default_rng(5)
    graphs = []
    for t in range(150):
        g, _ = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 10)), strand="+-."[t % 3])
        V = int(g["V"])
        dup = [e for e in g["edges"] if e[0] > 0 and e[1] < V - 1 and rng.random() < 0.2]
        g["edges"] = list(g["edges"]) + [(e[0], e[1], float(e[2]) * 0.5 + 1.0) + tuple(e[3:]) for e in dup]
        graphs.append(g)
    pg = PackedGraphs.from_graphs(graphs)
    n_par = 0                                                           # parallel edges are there
    for g in range(pg.n):
        one = pg.select(np.array([g]))
        src = np.repeat(np.arange(int(one.g_nv[0])), np.diff(one.vertex_offset))
        n_par += len(src) - len(set(zip(src.tolist(), one.edge_target.tolist())))
    assert n_par > 50, n_par
    s = check_against_oracle(pg, random_extras(pg, rng))
    assert s["complete"] > 100, s


# ---- the ABI surface
NEW = ("ald_batch_features_all", "ald_batch_features_table", "ald_batch_features_stats")


def test_new_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(common.ROOT, "include", "aletsch_decomp.h")).read()
    lib = A.load_library()
    out = os.popen(f"nm -D --defined-only {A.library_path()}").read()
    for n in NEW:
        assert n + "(" in hdr.replace(" ", "").replace("\n", "") or ("%s(" % n) in hdr, n
        assert hasattr(lib, n) and (" " + n + "\n") in out, n
    assert "trst_feature" not in out                                    # the kernel's host stub stays local


def test_null_arguments_and_no_device():
    lib = A.load_library()
    assert lib.ald_batch_features_all(None, None) == -1
    assert lib.ald_batch_features_table(None, None, None, None, None, None) == -1
    assert lib.ald_batch_features_stats(None, None, None, None, None) == -1
    import torch
    if not torch.cuda.is_available():                                   # without a device there is no batch to compute on
        with pytest.raises(A.DecompError) as e:
            A.DecompBatch(0)
        assert e.value.code == -2


def test_batch_extras_helper():
    ex = [A.GraphExtras.from_arrays(gr_reads=3, boundary_loss1=np.arange(4.0), unbridge_coming_count=np.arange(4)), None,
          A.GraphExtras.from_arrays(gr_subgraph=2, boundary_loss1=np.ones(3))]
    bx = A.BatchExtras.from_graph_extras(ex, [4, 2, 3])
    assert list(bx.arrays["boundary_loss1"]) == [0, 1, 2, 3, 0, 0, 1, 1, 1]
    assert list(bx.arrays["unbridge_coming_count"]) == [0, 1, 2, 3, 0, 0, 0, 0, 0]
    assert list(bx.arrays["gr_reads"]) == [3, 0, 0] and list(bx.arrays["gr_subgraph"]) == [0, 0, 2]
    assert not bx.boundary_loss2 and "boundary_loss2" not in bx.arrays
    assert A.FEATURE_DTYPE.itemsize == C.sizeof(A.TrstFeatures) == 296


def test_feature_kernel_has_no_spill_in_narrowed_exec():
    """the feature kernel's assembly (`make isa`: build/csrc/isa_other/) through tools/isa_spill_audit.py; no scratch either"""
    import shutil
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    s = os.path.join(common.ROOT, "build", "csrc", "isa_other", "trst_features.s")
    subprocess.run(["make", "-C", os.path.join(common.ROOT, "aletsch_amd", "csrc"), "../../build/csrc/isa_other/trst_features.s"],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "isa_spill_audit.py"), s], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    txt = open(s).read()
    assert ".private_segment_fixed_size: 0" in txt
