"""CPU tier of the feature block of RAW graphs on the device (ald_batch_features_all_ex, ALD_FEAT_RAW_ON_DEVICE): the raw instantiation of
the kernel's per-graph routine (aletsch_amd/csrc/trst_features_dev.h: boundary grouping into an overlay of the wire edges, then the rows),
compiled with g++ under -DALD_EMU (tests/feature_emu_raw) and fed graphs as assembler::assemble(gx, px, sid) receives them plus the
oracle's paths, against the oracle: its pre-steps (ora_pre_assemble) give the grouped graph, its restatement of
scallop::update_trst_features + unique_junc on that graph gives the rows.  Every field of every complete row bit for bit, the complete
flags, graph_rc; junction lists in LDS and in the scratch.  And the ABI surface of the new entry point."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import aletsch_amd as A
import common
from aletsch_amd.native import GraphView, PhaseView
from aletsch_amd.packed import PackedGraphs

_FEMUR = None
INV_OTHER = 109                                                       # ALD_ST_INVARIANT + ALD_INV_OTHER


def femur_lib():
    global _FEMUR
    if _FEMUR is None:
        path = os.path.join(common.ROOT, "tests", "_build", "libfeature_emu_raw.so")
        src = [os.path.join(common.ROOT, "aletsch_amd", "csrc", f) for f in ("trst_features_dev.h", "decomp_common.h", "host_pack.h")] + \
              [os.path.join(common.ROOT, "tests", "feature_emu_raw", "feature_emu_raw.cc")]
        if not os.path.exists(path) or any(os.path.getmtime(f) > os.path.getmtime(path) for f in src):
            subprocess.run(["make", "-C", os.path.join(common.ROOT, "tests", "feature_emu_raw")], check=True, stdout=subprocess.DEVNULL)
        L = C.CDLL(path)
        L.femur_batch_new.restype = C.c_void_p
        L.femur_batch_free.argtypes = [C.c_void_p]
        L.femur_batch_add_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        L.femur_features.argtypes = [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 4
        _FEMUR = L
    return _FEMUR


def emu_features_raw(items, res, extras=None, lds_words=4096):
    """items: [(single-graph PackedGraphs, phases, dist)], staged RAW; the device routine on one lane over the paths of `res`
    -> (rows, complete, graph_rc, live edge counts of the overlay)"""
    L = femur_lib()
    B = C.c_void_p(L.femur_batch_new())
    try:
        for pg, phases, dist in items:
            gv = GraphView.from_packed(pg, 0); pv = PhaseView.from_lists(phases)
            assert L.femur_batch_add_raw(B, C.byref(gv), C.byref(pv), C.c_int32(dist)) == 0
        n = len(items)
        path_offset = np.asarray(res.path_offset, np.int64); pv_offset = np.asarray(res.pv_offset, np.int64)
        pv = np.ascontiguousarray(res.path_vertices, np.int32)
        m = int(path_offset[-1])
        rows = np.zeros(max(m, 1), A.FEATURE_DTYPE); comp = np.zeros(max(m, 1), np.int32); rc = np.full(n, -77, np.int32); live = np.zeros(n, np.int32)
        p = lambda a: C.c_void_p(a.ctypes.data)
        assert L.femur_features(B, p(path_offset), p(pv_offset), p(pv), C.byref(extras) if extras is not None else None, C.c_int32(lds_words),
                                p(rows), p(comp), p(rc), p(live)) == 0
    finally:
        L.femur_batch_free(B)
    return rows[:m], comp[:m], rc, live


def _oracle_pre():
    O = common.oracle_lib()
    O.ora_pre_assemble.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    O.ora_staged_view.argtypes = [C.c_void_p, C.c_void_p]; O.ora_staged_free.argtypes = [C.c_void_p]
    O.ora_staged_boundary_maps.argtypes = [C.c_void_p] * 5
    return O


def raw_item(g, phases, rng, dist):
    """graph dict -> single-graph PackedGraphs the way test_pre_steps_cpu.py hands it over: the listing order is the creation order"""
    pg = PackedGraphs.from_graphs([g])
    pg.edge_rank = np.array(sorted(range(len(g["edges"])), key=lambda k: (g["edges"][k][0], g["edges"][k][1])), np.int32)
    pg.edge_count = (pg.sample_counts() + rng.integers(0, 3, pg.edge_target.size)).astype(np.int32)
    return pg, phases, dist


def raw_draw(seed, n_graphs):
    """-> kept items, their graph dicts, the oracle's staged graphs, (smap, tmap) per kept graph, number of graphs the oracle's pre-steps asserted on"""
    rng = np.random.default_rng(seed)
    O = _oracle_pre()
    items, dicts, staged, maps = [], [], [], []; n_assert = 0
    for t in range(n_graphs):
        g, phases = common.gene_like_raw(rng, n_runs=int(rng.integers(3, 10)), strand="+-."[t % 3])
        it = raw_item(g, phases, rng, int(rng.choice([10000, 10000, 150, 0])))
        want, sm, tm, rc = A.pre_assemble(it[0], phases, it[2], _lib=O, _prefix="ora")
        if rc:
            n_assert += 1; continue
        items.append(it); dicts.append(g); staged.append(want); maps.append((sm, tm))
    return items, dicts, staged, maps, n_assert


def random_extras(g_nv, rng):
    TV = int(np.sum(g_nv)); n = len(g_nv)
    return A.BatchExtras.from_arrays(boundary_loss1=rng.random(TV), boundary_loss2=rng.random(TV), boundary_loss3=rng.random(TV), boundary_merged_loss=rng.random(TV),
                                     unbridge_leaving_count=rng.integers(0, 9, TV), unbridge_leaving_ratio=rng.random(TV),
                                     unbridge_coming_count=rng.integers(0, 9, TV), unbridge_coming_ratio=rng.random(TV),
                                     gr_reads=rng.integers(1, 10000, n), gr_subgraph=rng.integers(0, 4, n))


def per_graph_extras(g_nv, bx):
    off = np.concatenate([[0], np.cumsum(g_nv)])
    out = []
    for g in range(len(g_nv)):
        kw = {k: v[off[g]:off[g + 1]] for k, v in bx.arrays.items() if k not in ("gr_reads", "gr_subgraph")}
        out.append(A.GraphExtras.from_arrays(gr_reads=int(bx.arrays["gr_reads"][g]), gr_subgraph=int(bx.arrays["gr_subgraph"][g]), **kw))
    return out


def check_raw_against_oracle(items, dicts, staged, extras):
    """the emulated raw routine on the RAW graphs + the oracle's paths == the oracle's features of the oracle's STAGED graphs"""
    batch = PackedGraphs.concat(staged)
    g_nv = np.array([int(it[0].g_nv[0]) for it in items])
    assert np.array_equal(g_nv, batch.g_nv)                           # the grouping renumbers nothing: extras and paths carry over
    res, want = common.oracle_features(batch, per_graph_extras(g_nv, extras) if extras is not None else None)
    stats = dict(complete=0, single=0, asserted=0, overlay_read=0, fewer_edges=0)
    tables = [emu_features_raw(items, res, extras, lds) for lds in (4096, 0)]          # junction lists in LDS / all in the scratch
    for ti, (rows, comp, rc, live) in enumerate(tables):
        for g in range(len(items)):
            wf, wc, wbad = want[g]
            assert (rc[g] != 0) == wbad and rc[g] in (0, INV_OTHER), (g, rc[g], wbad)
            r0, r1 = int(res.path_offset[g]), int(res.path_offset[g + 1])
            assert r1 - r0 == len(wc)
            if r1 > r0:
                assert live[g] == int(batch.g_ne[g]), (g, live[g], int(batch.g_ne[g]))       # the overlay's live count is the staged graph's E
            if wbad:
                stats["asserted"] += 1; continue
            assert np.array_equal(comp[r0:r1], wc), g
            w_in = {(e[0], e[1]): float(e[2]) for e in dicts[g]["edges"]}
            fewer = False
            for k in range(len(wc)):
                d = {x: rows[r0 + k][x].item() for x in A.FEATURE_DTYPE.names}
                fewer = fewer or d["gr_edges"] < int(items[g][0].g_ne[0])
                if wc[k]:
                    bad = {x: (d[x], wf[k][x]) for x in d if np.float64(d[x]).tobytes() != np.float64(wf[k][x]).tobytes() and d[x] != wf[k][x]}
                    assert d == wf[k], (g, k, bad)
                    if ti == 0:
                        stats["complete"] += 1
                        first = int(res.path_vertices[int(res.pv_offset[r0 + k]) + 1])
                        stats["overlay_read"] += int(d["start_weight"] != w_in[(0, first)])
                else:
                    for x in ("gr_vertices", "gr_edges", "gr_reads", "gr_subgraph", "num_vertices", "num_edges", "max_mid_exon_len"):
                        assert d[x] == wf[k][x]
                    if ti == 0:
                        stats["single"] += 1
            if ti == 0:
                stats["fewer_edges"] += int(fewer)
    for name in A.FEATURE_DTYPE.names:                                     # both placements give the same bits
        a, b = tables[0][0][name], tables[1][0][name]
        assert a.tobytes() == b.tobytes(), name
    assert np.array_equal(tables[0][2], tables[1][2])
    return stats


def test_raw_routine_matches_oracle_on_gene_like_graphs():
    N = 300
    items, dicts, staged, maps, n_assert = raw_draw(1078, N)
    assert n_assert < 0.2 * N, n_assert
    rng = np.random.default_rng(4)
    s = check_raw_against_oracle(items, dicts, staged, random_extras([int(it[0].g_nv[0]) for it in items], rng))
    n_start = sum(1 for sm, tm in maps if sm); n_end = sum(1 for sm, tm in maps if tm)
    n_both = sum(1 for sm, tm in maps if sm and tm); n_none = sum(1 for sm, tm in maps if not sm and not tm)
    census = dict(start=n_start, end=n_end, both=n_both, none=n_none, **s)
    print(census)
    assert n_start >= 30 and n_end >= 30 and n_both >= 10 and n_none >= 10, census
    assert s["overlay_read"] >= 50 and s["fewer_edges"] >= 30 and s["complete"] > 300, census


def fan_graph(rng, width=70):
    """A run of `width` touching one-base vertices with a source edge to each (width - 1 start boundaries fold into the first, the chain
    edge 1 -> 2 takes one addition per fold), a few spliced exons, and the mirror image into the sink: wider than a wave on purpose.
    Weights are not integers, so every sum depends on the order of its additions."""
    W = width
    lpos = [1000]; rpos = [1000]
    for i in range(W):
        lpos.append(1000 + i); rpos.append(1001 + i)
    mid = []
    pos = 1000 + W + 500
    for i in range(4):
        mid.append(len(lpos)); lpos.append(pos); rpos.append(pos + 120); pos += 120 + 300
    e0 = len(lpos)
    for i in range(W):
        lpos.append(pos + i); rpos.append(pos + i + 1)
    V = len(lpos) + 1; lpos.append(pos + W); rpos.append(pos + W)
    wt = lambda: float(rng.random() * 30 + 0.37)
    info = lambda: {0: float(rng.integers(1, 30)), int(rng.integers(1, 6)): float(rng.integers(1, 30))}
    edges = []
    add = lambda s, t, st=0: edges.append((s, t, wt(), st, info()))
    for i in range(1, W + 1):
        add(0, i)
    for i in range(1, W):
        add(i, i + 1)
    add(W, mid[0], 1); add(W // 2, mid[0], 1); add(W // 3, mid[1], 1); add(5, mid[0], 1)
    add(mid[0], mid[1], 1); add(mid[1], mid[2], 1); add(mid[0], mid[2], 1); add(mid[2], mid[3], 1); add(mid[1], mid[3], 1)
    add(mid[3], e0, 1); add(mid[2], e0 + W // 2, 1); add(mid[3], e0 + W // 3, 1); add(mid[1], e0 + W - 5, 1)
    for i in range(e0, e0 + W - 1):
        add(i, i + 1)
    for i in range(e0, e0 + W):
        add(i, V - 1)
    edges = [edges[i] for i in rng.permutation(len(edges))]
    vw = [0.0] + [float(rng.integers(1, 50)) for _ in range(V - 2)] + [0.0]
    g = dict(V=V, edges=edges, vw=vw, lpos=lpos, rpos=rpos, strand="+")
    phases = [([lpos[1], rpos[W], lpos[mid[0]], rpos[mid[0]]], 3), ([lpos[mid[2]], rpos[mid[2]], lpos[mid[3]], rpos[mid[3]]], 2)]
    return g, phases


def fan_items(rng):
    out = []
    for dist in (10000, 10000, 30, 0):
        g, phases = fan_graph(rng)
        out.append((g, raw_item(g, phases, rng, dist)))
    return out


def test_seventy_wide_fans_on_both_sides():
    rng = np.random.default_rng(70)
    O = _oracle_pre()
    items, dicts, staged = [], [], []
    for g, it in fan_items(rng):
        want, sm, tm, rc = A.pre_assemble(it[0], it[1], it[2], _lib=O, _prefix="ora")
        assert rc == 0
        if it[2] == 10000:
            assert len(sm) == 69 and len(tm) == 69 and int(want.g_ne[0]) == int(it[0].g_ne[0]) - 138
        if it[2] == 0:
            assert not sm and not tm
        items.append(it); dicts.append(g); staged.append(want)
    s = check_raw_against_oracle(items, dicts, staged, random_extras([int(it[0].g_nv[0]) for it in items], rng))
    assert s["complete"] >= 4 and s["overlay_read"] >= 2 and s["fewer_edges"] >= 3, s


# ---- the ABI surface
def test_ex_entry_point_is_declared_and_exported():
    hdr = open(os.path.join(common.ROOT, "include", "aletsch_decomp.h")).read()
    lib = A.load_library()
    out = os.popen(f"nm -D --defined-only {A.library_path()}").read()
    assert "ald_batch_features_all_ex(" in hdr.replace(" ", "") and "#define ALD_FEAT_RAW_ON_DEVICE 1u" in hdr
    assert hasattr(lib, "ald_batch_features_all_ex") and " ald_batch_features_all_ex\n" in out
    assert "trst_feature" not in out                                    # the kernel's host stub stays local


def test_ex_null_batch_and_unknown_flags():
    lib = A.load_library()
    assert lib.ald_batch_features_all_ex(None, None, 1) == -1
    assert lib.ald_batch_features_all_ex(None, None, 2) == -1
    import torch
    if torch.cuda.is_available():                                       # a valid call path: the flag check comes before the state check
        with A.DecompBatch(0) as b:
            b.upload(); b.run(); b.download()
            assert lib.ald_batch_features_all_ex(b._h, None, 2) == -1
            assert lib.ald_batch_features_all_ex(b._h, None, 3) == -1
            assert lib.ald_batch_features_all_ex(b._h, None, 1) == 0
    else:                                                               # without a device there is no batch to call it on
        with pytest.raises(A.DecompError) as e:
            A.DecompBatch(0)
        assert e.value.code == -2


def test_feature_kernel_with_the_raw_instantiation_uses_no_scratch():
    """every kernel of trst_features.s (`make isa`: build/csrc/isa_other/) has no private segment, and tools/isa_spill_audit.py is clean"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc: the assembly cannot be produced here")
    s = os.path.join(common.ROOT, "build", "csrc", "isa_other", "trst_features.s")
    subprocess.run(["make", "-C", os.path.join(common.ROOT, "aletsch_amd", "csrc"), "../../build/csrc/isa_other/trst_features.s"],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, os.path.join(common.ROOT, "tools", "isa_spill_audit.py"), s], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    sizes = [ln.split(":")[1].strip() for ln in open(s) if ".private_segment_fixed_size:" in ln]
    assert sizes and all(x == "0" for x in sizes), sizes
